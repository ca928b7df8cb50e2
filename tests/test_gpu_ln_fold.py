"""The LayerNorm-folded GEMM seams (norm2 -> fc1 of both proxy blocks, norm_img -> proxy_proj) against float64, OFF zero-mean rows.

The forward never forms LayerNorm(x): the producer GEMM leaves per-row, per-32-column-tile fp32 partials of its output, the consumer
GEMM (k_gemm32 / k_gemm64 / k_gemm64x / k_gemm128x, or the fused k_mlp) turns them into (mean, rstd) and applies the normalisation
around its product.  Rows whose mean is large against their spread are where such a fold cancels; every other test of the suite
feeds the seams rows with |mean| / sigma <= ~1.

The yardstick of (b) - (d): the reference formula (layer_norm, then linear) evaluated in torch-CPU float32 on the same inputs loses
e_ref = max |y_ref32 - y64|; the kernel passes with max |y_gpu - y64| <= 4 e_ref.  An fp32 LayerNorm's own error grows with
mean / sigma, so no fixed absolute bar fits the axis; 4 is twice the worst ratio (1.44 at mean / sigma = 1000) that a centred fp32
restatement of the fold (tile sums and tile M2 combined by Chan's formula, x - mean formed before the product) shows on the CPU over
mean / sigma = 0 .. 1000, rounded up for the dropped terms of the six-term split product.  It is not taken from the kernels.

Every case prints one line "kernel role R N C mean/sigma sigma e_ref err ratio control"; with LN_FOLD_REPORT=<file> the lines are
appended to that file (profiles/ln_fold_conditioning.txt is made that way).  control = the same rows normalised in float64, rounded to
fp32 and sent through the plain ptx_linear, in units of e_ref: what the GEMM alone costs."""
import contextlib
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

EPS = 1e-5
MARGIN = 4.0
RATIOS = (0, 1, 3, 10, 30, 100)


def _report(kernel, role, R, N, C, ratio, sigma, e_ref, err, control=None, note=""):
    line = (f"{kernel:<12s} {role:<22s} R={R:<5d} N={N:<5d} C={C:<4d} mean/sigma={ratio:<8.4g} sigma={sigma:<6g} e_ref={e_ref:.3e} "
            f"err={err:.3e} ratio={err / e_ref:7.3f} control={'   -   ' if control is None else f'{control / e_ref:7.3f}'} {note}")
    print(line)
    path = os.environ.get("LN_FOLD_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


# ---- launch_gemm's kernel choice (csrc/gemm.hip, launch_gemm), restated so that every case below names the kernel it reaches ------
def _cdiv(a, b):
    return (a + b - 1) // b


def gemm_kernel(R, N, K, policy):
    """The kernel a single-group fp32 launch of (R, N, K) runs on under ptx_gemm_policy(policy), policy in (0, 1)."""
    if policy == 1 and K % 256 == 0 and K <= 4096:
        return "k_gemm128x"
    tiles32 = _cdiv(R, 32) * _cdiv(N, 32)
    if tiles32 >= 1024:
        return "k_gemm64x" if K % 128 == 0 and K // 128 in (1, 2, 4, 8, 6, 12, 16, 32) else "k_gemm64"
    nk, sk = _cdiv(K, 32), 1
    while sk < 4 and tiles32 * sk < 4096 and nk >= 4 * sk:
        sk *= 2
    return f"k_gemm32/SK{sk}"


# ============================================================================================ (a) producer partials
# (R, N, K, policy, kernel).  N % 128 in (0, 64] puts a 32-column quadrant of a 128-column tile wholly past N; N % 64 in (0, 32]
# (N = 32, 96) does the same to the right-hand wave of a 64-column tile.  The 64-column kernels are only chosen from 1024 tiles of
# 32 x 32 on, which N = 96 reaches at R >= 10912: the two R = 11000 cases are there for that.
PRODUCER_CASES = [
    # k_gemm32, K = 64: two K steps, one wave per tile
    (1, 32, 64, 0, "k_gemm32/SK1"), (33, 96, 64, 0, "k_gemm32/SK1"), (129, 320, 64, 0, "k_gemm32/SK1"), (33, 448, 64, 1, "k_gemm32/SK1"),
    # k_gemm32, K = 160: five K steps over two waves
    (1, 64, 160, 0, "k_gemm32/SK2"), (129, 192, 160, 0, "k_gemm32/SK2"), (33, 512, 160, 0, "k_gemm32/SK2"), (129, 96, 160, 1, "k_gemm32/SK2"),
    # k_gemm32, K = 256 / 512 below 1024 tiles: four waves
    (33, 256, 256, 0, "k_gemm32/SK4"), (129, 448, 512, 0, "k_gemm32/SK4"), (1, 32, 512, 0, "k_gemm32/SK4"), (2000, 96, 256, 0, "k_gemm32/SK4"),
    (129, 320, 256, 0, "k_gemm32/SK4"),
    # k_gemm64 (fp32 matrix instruction): >= 1024 tiles, K no multiple of 128
    (4100, 256, 64, 0, "k_gemm64"), (4100, 320, 160, 0, "k_gemm64"), (4100, 448, 160, 1, "k_gemm64"), (4100, 512, 64, 0, "k_gemm64"),
    (11000, 96, 64, 0, "k_gemm64"),
    # k_gemm64x (split operands): >= 1024 tiles, K = 256 / 512, small-tile policy
    (4100, 256, 256, 0, "k_gemm64x"), (4100, 320, 512, 0, "k_gemm64x"), (4100, 448, 256, 0, "k_gemm64x"), (4100, 512, 512, 0, "k_gemm64x"),
    (11000, 96, 256, 0, "k_gemm64x"),
    # k_gemm128x: K = 256 / 512 with the large tile forced, at every row count
    (1, 32, 256, 1, "k_gemm128x"), (33, 64, 512, 1, "k_gemm128x"), (129, 192, 256, 1, "k_gemm128x"), (2000, 320, 512, 1, "k_gemm128x"),
    (4100, 448, 256, 1, "k_gemm128x"), (2000, 96, 256, 1, "k_gemm128x"), (4100, 512, 512, 1, "k_gemm128x"), (129, 256, 512, 1, "k_gemm128x"),
    (33, 32, 256, 1, "k_gemm128x"), (129, 320, 256, 1, "k_gemm128x"), (2000, 192, 512, 1, "k_gemm128x"), (4100, 64, 256, 1, "k_gemm128x"),
    (33, 448, 512, 1, "k_gemm128x"), (1, 96, 512, 1, "k_gemm128x"), (2000, 32, 256, 1, "k_gemm128x"), (4100, 96, 512, 1, "k_gemm128x"),
    (129, 64, 256, 1, "k_gemm128x"),
    # widths that are no multiple of 32: the last tile's mean and M2 run over N % 32 columns
    (129, 100, 64, 0, "k_gemm32/SK1"), (33, 200, 256, 0, "k_gemm32/SK4"), (4100, 300, 160, 0, "k_gemm64"), (4100, 300, 256, 0, "k_gemm64x"),
    (2000, 100, 256, 1, "k_gemm128x"), (129, 200, 512, 1, "k_gemm128x"), (4100, 44, 256, 1, "k_gemm128x"),
]


@pytest.mark.parametrize("R,N,K,policy,kernel", PRODUCER_CASES)
def test_producer_partials(R, N, K, policy, kernel):
    """y at ptx_linear's bar; every partial (sum, M2 about the tile's own mean) against the float64 statistics of the kernel's OWN fp32
    y over the tile's valid columns; nothing written outside (row < R, tile < parts).

    Bounds (derived, not measured): a 32-term fp32 sum in any order is within 31 * 2^-24 * sum |term| to first order; twice that,
    32 * 2^-23 * sum |v|, for the sum.  M2 = sum (v - m~)^2 with m~ the fp32 tile mean: each (v - m~)^2 carries three roundings and the
    sum 31 more, < 32 * 2^-23 * M2; m~ itself is off by at most 32 * 2^-24 * sum |v| / n, which moves M2 by n (m~ - m)^2 <= 2^-38 *
    (sum |v|)^2 / n <= 2^-38 sum v^2 (Cauchy-Schwarz).  So |M2 - M2_64| <= 32 * 2^-23 * M2_64 + 2^-32 * sum v^2, which is never wider
    than 32 * 2^-23 * sum v^2.

    On a kernel without the `part < parts` guard a quadrant past N writes (0, 0) over partial 0 of the next row (racing its rightful
    writer) and, on the last row, behind the buffer: the float64 comparison of that partial and the sentinels reject both."""
    from tests.gpu_util import GUARD_WORD, gemm_policy, linear_ln_partials
    assert gemm_kernel(R, N, K, policy) == kernel
    g = torch.Generator().manual_seed(7000 + R + 3 * N + 5 * K + policy)
    x = torch.randn(R, K, generator=g)
    w = torch.randn(N, K, generator=g) * 0.1
    b = torch.randn(N, generator=g) + 2.0                   # an offset: the sums do not hover around zero
    res = torch.randn(R, N, generator=g) if (R + N + K) % 2 else None
    with gemm_policy(policy):
        y, lnp, guard = linear_ln_partials(x.cuda(), w.cuda(), b.cuda(), None if res is None else res.cuda())
    torch.cuda.synchronize()
    y, lnp = y.cpu().double(), lnp.cpu().double()
    y64 = x.double() @ w.double().t() + b.double()
    bound = 4e-6 * (x.double().abs() @ w.double().abs().t() + b.double().abs()) + 1e-30
    if res is not None:
        y64, bound = y64 + res.double(), bound + 4e-6 * res.double().abs()
    worst = ((y - y64).abs() / bound).max().item()
    assert worst <= 1.0, f"y: error / bound = {worst:.3f}"
    assert bool((guard.cpu() == GUARD_WORD).all()), "words behind the partials buffer were written"
    parts = (N + 31) // 32
    assert lnp.shape == (R, parts, 2)
    assert not bool(torch.isnan(lnp).any()), f"{int(torch.isnan(lnp).any(-1).sum())} partials never written"
    pad = parts * 32 - N
    yp = F.pad(y, (0, pad)).view(R, parts, 32)
    valid = (torch.arange(parts * 32).view(parts, 32) < N).double()          # (parts, 32)
    cnt = valid.sum(-1)                                                        # (parts)
    s1 = (yp * valid).sum(-1)
    sabs = (yp.abs() * valid).sum(-1)
    ssq = (yp * yp * valid).sum(-1)
    m2 = (((yp - (s1 / cnt)[..., None]) ** 2) * valid).sum(-1)
    u = 32 * 2.0 ** -23
    e1 = ((lnp[..., 0] - s1).abs() / (u * sabs + 1e-300)).max().item()
    e2 = ((lnp[..., 1] - m2).abs() / (u * m2 + 2.0 ** -32 * ssq + 1e-300)).max().item()
    print(f"{kernel} R={R} N={N} K={K} policy={policy}: y {worst:.3f}  sum {e1:.3f}  M2 {e2:.3f} of their bounds")
    assert e1 <= 1.0, f"tile sums: error / bound = {e1:.3f}"
    assert e2 <= 1.0, f"tile M2: error / bound = {e2:.3f}"


# ============================================================================================ (b) seam conditioning, operator level
# (C, R, N, gelu, policy, consumer kernel): each consumer kernel sees the whole mean / sigma x sigma grid at least once.  C = 160 is
# there because k_gemm64 (fp32 instruction) is only chosen where K is no multiple of 128.
SEAM_GROUPS = [
    (256, 65, 256, 0, 0, "k_gemm32"),
    (512, 33, 2048, 1, 0, "k_gemm32"),
    (256, 1100, 1024, 1, 0, "k_gemm64x"),
    (512, 600, 2048, 0, 0, "k_gemm64x"),
    (160, 1100, 1024, 1, 0, "k_gemm64"),
    (512, 700, 2048, 1, 1, "k_gemm128x"),
    (256, 300, 256, 0, 1, "k_gemm128x"),
]


def _seam_operands(C, R, N, ratio, sigma, seed):
    g = torch.Generator().manual_seed(seed)
    rows = (torch.randn(R, C, generator=g) + float(ratio)) * sigma           # no row is constant: randn has full spread
    k = 1.0 / np.sqrt(C)
    w = (torch.rand(N, C, generator=g) * 2 - 1) * k
    b = (torch.rand(N, generator=g) * 2 - 1) * 0.1
    gamma = 1.0 + (torch.rand(C, generator=g) * 2 - 1) * 0.1
    beta = (torch.rand(C, generator=g) * 2 - 1) * 0.1
    return rows, w, b, gamma, beta


@contextlib.contextmanager
def _one_thread():
    """The float32 reference runs on ONE thread: e_ref is a maximum over a float32 evaluation, whose summation order would otherwise
    follow the host's core count (the bar of a case is 4 e_ref, and the closest case sits at 3.8)."""
    prev = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        yield
    finally:
        torch.set_num_threads(prev)


def _ln_linear_ref(x, w, b, gamma, beta, gelu):
    y = F.linear(F.layer_norm(x, (x.shape[-1],), gamma, beta, EPS), w, b)
    return F.gelu(y) if gelu else y


def _seam_case(C, R, N, gelu, policy, ratio, sigma, real_projection=False, seed=None):
    """Producer -> consumer on the GPU; returns (raw rows as the consumer read them, y_gpu, operands)."""
    from tests.gpu_util import gemm_policy, linear_ln_partials, ln_linear
    if seed is None:
        seed = 9000 + C + R + N + 17 * int(ratio) + int(np.log10(sigma)) + 3 * policy
    rows, w, b, gamma, beta = _seam_operands(C, R, N, ratio, sigma, seed)
    with gemm_policy(policy):
        if real_projection:     # a projection of zero-mean rows whose bias is m 1 + 0.1 u
            g = torch.Generator().manual_seed(77)
            a = torch.randn(R, C, generator=g) * sigma
            wp = (torch.rand(C, C, generator=g) * 2 - 1) / np.sqrt(C)
            bp = (float(ratio) + (torch.rand(C, generator=g) * 2 - 1) * 0.1) * sigma / np.sqrt(3.0)
            raw, lnp, _ = linear_ln_partials(a.cuda(), wp.cuda(), bp.cuda())
        else:                   # identity producer: y = rows exactly (products with 1 and 0 are exact in every kernel)
            raw, lnp, _ = linear_ln_partials(rows.cuda(), torch.eye(C).cuda())
        y = ln_linear(raw, lnp, w.cuda(), gamma.cuda(), beta.cuda(), b.cuda(), EPS, gelu)
    torch.cuda.synchronize()
    raw = raw.cpu()
    if not real_projection:
        assert torch.equal(raw, rows)
    return raw, y.cpu(), (w, b, gamma, beta)


def _measure(raw, y, ops, gelu):
    from tests.gpu_util import linear
    w, b, gamma, beta = ops
    y64 = _ln_linear_ref(raw.double(), w.double(), b.double(), gamma.double(), beta.double(), gelu)
    with _one_thread():
        y32 = _ln_linear_ref(raw, w, b, gamma, beta, gelu)
    e_ref = (y32.double() - y64).abs().max().item()
    err = (y.double() - y64).abs().max().item()
    xn = F.layer_norm(raw.double(), (raw.shape[-1],), gamma.double(), beta.double(), EPS).float()
    yc = linear(xn.cuda(), w.cuda(), b.cuda(), None, gelu).cpu()
    ctl = (yc.double() - y64).abs().max().item()
    rd = raw.double()
    seen = (rd.mean(-1).abs() / rd.std(-1, unbiased=False)).median().item()
    return e_ref, err, ctl, seen


@pytest.mark.parametrize("sigma", [1e-3, 1.0, 1e3])
@pytest.mark.parametrize("ratio", RATIOS)
@pytest.mark.parametrize("C,R,N,gelu,policy,kernel", SEAM_GROUPS)
def test_seam_conditioning(C, R, N, gelu, policy, kernel, ratio, sigma):
    raw, y, ops = _seam_case(C, R, N, gelu, policy, ratio, sigma)
    e_ref, err, ctl, seen = _measure(raw, y, ops, gelu)
    _report(kernel, "consumer" + ("+gelu" if gelu else ""), R, N, C, seen, sigma, e_ref, err, ctl)
    assert err <= MARGIN * e_ref, f"max |y - y64| = {err:.3e} = {err / e_ref:.2f} e_ref (e_ref = {e_ref:.3e})"


@pytest.mark.parametrize("ratio", RATIOS)
@pytest.mark.parametrize("policy,kernel", [(0, "k_gemm64x"), (1, "k_gemm128x")])
def test_seam_conditioning_behind_a_real_projection(policy, kernel, ratio):
    """The rows come out of a projection (256 -> 256, on k_gemm32 under policy 0 and on k_gemm128x under policy 1) with a bias of
    m 1 + 0.1 u; the consumer reads what that launch wrote."""
    C, R, N = 256, 1100, 1024
    raw, y, ops = _seam_case(C, R, N, 1, policy, ratio, 1.0, real_projection=True)
    e_ref, err, ctl, seen = _measure(raw, y, ops, 1)
    _report(kernel, "proj -> consumer+gelu", R, N, C, seen, 1.0, e_ref, err, ctl)
    assert err <= MARGIN * e_ref, f"max |y - y64| = {err:.3e} = {err / e_ref:.2f} e_ref (e_ref = {e_ref:.3e})"


def test_seam_launch_is_bit_identical_on_both_tile_sizes():
    """k_gemm64x and k_gemm128x form x - mean the same way and add the same products in the same order: the tile policy cannot change a
    forward's output at a seam either (test_default_policy_picks_the_tile_by_launch_size holds that for launches without one)."""
    assert gemm_kernel(1100, 1024, 256, 0) == "k_gemm64x" and gemm_kernel(1100, 1024, 256, 1) == "k_gemm128x"
    for ratio in (0, 10, 100):
        raw_small, y_small, _ = _seam_case(256, 1100, 1024, 1, 0, ratio, 1.0, seed=4242)
        raw_big, y_big, _ = _seam_case(256, 1100, 1024, 1, 1, ratio, 1.0, seed=4242)
        assert torch.equal(raw_big, raw_small) and torch.equal(y_big, y_small), ratio


@pytest.mark.parametrize("C", [0, 16, 48, 100, 544, 1024])
def test_consumer_rejects_widths_it_cannot_fold(C):
    """C a multiple of 32, at most 512 (sixteen partials per row): anything else is an error, not a launch."""
    from proxytransformation_amd import _abi
    lib = _abi.lib()
    z = torch.zeros(4096, device="cuda")
    rc = lib.ptx_ln_linear(z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), None, EPS, 0, z.data_ptr(),
                           z.data_ptr(), z.numel() * 4, 1, 1, C, torch.cuda.current_stream().cuda_stream)
    assert rc != 0 and b"n_in" in lib.ptx_last_error()
    torch.cuda.synchronize()
    assert float(z.abs().max()) == 0.0


# ============================================================================================ (c) block level, the public ABI
# (name, C, grid_size, B, policy, consumer): R = B * M_keep rows.  The fused Mlp (C = 256) takes 32 rows x a quarter of the hidden units
# per work-group: a single-branch call has ceil(R / 32) * 4 of them, and launch_mlp picks the LITE form for 256 < that <= 400.
BLOCK_CONFIGS = [
    ("c256_small", 256, 4, 2, 0, "k_mlp"),                 # R = 64: 8 work-groups
    ("c256_lite", 256, 8, 10, 0, "k_mlp<LITE>"),           # R = 2560: 320 work-groups
    ("c512_small", 512, 4, 2, 0, "k_gemm32"),              # R = 64, fc1 2048 x 512: 128 tiles
    ("c512_large_64", 512, 8, 10, 0, "k_gemm64x"),         # R = 2560: 5120 tiles
    ("c512_large_128", 512, 8, 10, 1, "k_gemm128x"),
]
_block_cache = {}


def _block_setup(name, C, gs, B):
    from proxytransformation_amd.synth import PreshapeConfig
    from tests.gpu_util import Stages
    from tests.util import build_module
    if name not in _block_cache:
        _block_cache.clear()                                 # one module's workspace at a time
        cfg = PreshapeConfig(name, B=B, N=4096, grid_size=gs, dynamic_drop_radio=0.5, L=12, V=9, embed_dim=C, seed_base=6400)
        m, sd = build_module(cfg)
        m = m.cuda()
        _block_cache[name] = (cfg, m, sd, Stages(m, cfg.B, cfg.N, cfg.L, cfg.V))
    return _block_cache[name]


def _oracle_block(sd, which, cfg, pp, proxy, mask, dtype):
    """oracle.proxy_block's `out`, then the trailing norm / head / BatchNorm1d exactly as oracle.forward applies them."""
    from oracle import oracle
    sdt = {k: (torch.from_numpy(v).to(dtype) if v.dtype == np.float32 else torch.from_numpy(v)) for k, v in sd.items()}
    pre, norm, head, bn = (("textformer.0", "text_norm.0", "text_trans", "text_trans_norm") if which == 0 else
                           ("imgformer.0", "img_norm.0", "img_trans", "img_trans_norm"))
    with torch.no_grad():
        blk = oracle.proxy_block(sdt, pre, pp.to(dtype), proxy.to(dtype), mask, cfg.num_heads)
        guide = F.layer_norm(blk["out"], (cfg.embed_dim,), sdt[norm + ".weight"], sdt[norm + ".bias"], oracle.LN_EPS)
        out = oracle._bn1d_eval(sdt, bn, F.linear(guide, sdt[head + ".weight"], sdt[head + ".bias"]))
    return guide, out, blk["x1"]


@pytest.mark.parametrize("ratio", RATIOS)
@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("name,C,gs,B,policy,kernel", BLOCK_CONFIGS)
def test_block_conditioning(name, C, gs, B, policy, kernel, which, ratio):
    """ptx_proxy_block on point_proxy = randn + m rows: `guide` and the head output against the float64 oracle, bar 4 e_ref with e_ref
    from the float32 oracle on the same inputs.  The mean / sigma that reaches the seam is x1's (proj adds its own spread to the offset
    rows): reported from the float64 oracle's intermediate."""
    from tests.gpu_util import gemm_policy
    cfg, m, sd, st = _block_setup(name, C, gs, B)
    g = torch.Generator().manual_seed(6500 + 10 * int(ratio) + which)
    pp = torch.randn(cfg.B, cfg.M_keep, C, generator=g) + float(ratio)
    Lp = cfg.L if which == 0 else cfg.V
    proxy = torch.randn(cfg.B, Lp, C, generator=g)
    mask = None
    if which == 0:
        mask = torch.ones(cfg.B, Lp, dtype=torch.bool)
        mask[1, Lp - Lp // 3:] = False
    with gemm_policy(policy):
        head, guide = st.proxy_block(which, pp.cuda(), proxy.cuda(), None if mask is None else mask.to(torch.uint8).cuda())
    torch.cuda.synchronize()
    g64, h64, x1 = _oracle_block(sd, which, cfg, pp, proxy, mask, torch.float64)
    with _one_thread():
        g32, h32, _ = _oracle_block(sd, which, cfg, pp, proxy, mask, torch.float32)
    seen = (x1.mean(-1).abs() / x1.std(-1, unbiased=False)).median().item()
    R = cfg.B * cfg.M_keep
    bad = []
    for what, got, r64, r32 in (("guide", guide, g64, g32), ("head_out", head, h64, h32)):
        e_ref = (r32.double() - r64).abs().max().item()
        err = (got.cpu().double() - r64).abs().max().item()
        _report(kernel, f"block {which} {what}", R, 4 * C, C, seen, 1.0, e_ref, err, None, f"nominal={ratio}")
        if err > MARGIN * e_ref:
            bad.append(f"{what}: max |y - y64| = {err:.3e} = {err / e_ref:.2f} e_ref (e_ref = {e_ref:.3e})")
    assert not bad, "; ".join(bad)


# ============================================================================================ (d) the image seam's wiring in the forward
def test_forward_with_offset_image_rows():
    """norm_img -> proxy_proj inside the forward (the row offset of the image partials, the consumer's view of them): c_proj's bias is
    raised until its output rows sit at mean / sigma ~ 30.  The oracle's forward is float32 throughout (its clustering half is C code on
    float32), so the bars are the existing ones of the forward tests.

    This is a test of WIRING, not of conditioning: a constant added to c_proj's bias leaves LayerNorm of the rows unchanged in exact
    arithmetic, and the mean / sigma is asserted on the oracle's rows (the module's tables are prepared from the same state dict
    after it is loaded, so the GPU's rows carry the same offset).  Wrong partial rows or a wrong row offset give a wrong mean, and with
    rows 30 sigma off zero a wrong mean is an error of order 1 in img_guide / transform.  The same forward is then run in the
    reduced-precision compute mode, which sends the seam through the plain-bf16 variants of the centring kernels: centred rows cost
    bf16's 2^-9 of sigma, uncentred ones would cost 2^-9 of 30 sigma, so the existing bound of that mode (relative 5e-2 on the transforms,
    tests/test_gpu_edge_cases.py) has to hold here as it does on zero-mean rows."""
    from oracle import oracle
    from proxytransformation_amd.synth import PreshapeConfig, make_scene_batch
    from tests.gpu_util import t
    from tests.util import assert_close, build_module, oracle_kwargs
    cfg = PreshapeConfig("lnimg", B=3, N=12000, grid_size=6, dynamic_drop_radio=0.5, L=12, V=9, seed_base=6600)
    pts, text, mask, img = make_scene_batch(cfg)
    m, sd = build_module(cfg)
    sdt = {k: torch.from_numpy(v) for k, v in sd.items()}
    with torch.no_grad():
        rows = oracle.img_cproj(sdt, torch.from_numpy(img), cfg.num_heads).double()
    spread = rows.std(-1, unbiased=False).median().item()
    sd = dict(sd)
    sd["attn_pool2d.c_proj.bias"] = (sd["attn_pool2d.c_proj.bias"] + np.float32(30.0 * spread - rows.mean().item())).astype(np.float32)
    sdt = {k: torch.from_numpy(v) for k, v in sd.items()}
    with torch.no_grad():
        rows = oracle.img_cproj(sdt, torch.from_numpy(img), cfg.num_heads).double()
    seen = rows.mean(-1).abs() / rows.std(-1, unbiased=False)
    print(f"c_proj rows: mean / sigma = {seen.min().item():.1f} .. {seen.max().item():.1f}")
    assert 25.0 <= seen.median().item() <= 36.0 and seen.min().item() >= 10.0
    m.load_state_dict(sdt)
    m = m.cuda()
    ref = oracle.forward(sd, **oracle_kwargs(cfg), points=pts, text_feats=text, text_mask=mask, img_feat=img, num_threads=8)
    m._centers_override = torch.from_numpy(ref["centers"])
    d = m.forward_debug([t(p) for p in pts], {"text_feats": t(text), "text_token_mask": t(mask)}, t(img))
    for k in ("idx2", "order", "picks", "keep", "kidx", "drop_idx"):
        assert np.array_equal(d[k].cpu().numpy().astype(np.int64), ref[k]), k
    for k in ("img_proxy", "img_guide", "transform", "translate"):
        print(k, float(np.abs(d[k].cpu().numpy().reshape(ref[k].shape) - ref[k]).max()))
    assert_close(d["img_guide"].cpu().numpy(), ref["img_guide"], atol=5e-5, rtol=1e-5, what="img_guide")
    assert_close(d["transform"].cpu().numpy().reshape(ref["transform"].shape), ref["transform"], atol=5e-5, rtol=1e-5, what="transform")
    assert_close(d["translate"].cpu().numpy(), ref["translate"], atol=5e-5, rtol=1e-5, what="translate")
    for b in range(cfg.B):
        assert_close(d["outputs"][b].cpu().numpy(), ref["outputs"][b], atol=1e-4, what=f"scene {b}")
    m.compute_dtype = "bf16"
    d16 = m.forward_debug([t(p) for p in pts], {"text_feats": t(text), "text_token_mask": t(mask)}, t(img))
    for k in ("translate", "transform"):
        a, b16 = d[k].double(), d16[k].double()
        rel = float((a - b16).abs().max() / a.abs().max())
        print(k, "bf16 compute mode, relative to fp32:", rel)
        assert 1e-5 < rel < 5e-2, (k, rel)
