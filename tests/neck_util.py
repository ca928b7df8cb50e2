"""What the neck's test modules share: the rows of the union / score tests, the end-to-end levels and module, the near-tie count of a
pruning step, the end-to-end protocol itself, and the inputs and preconditions of tests/test_gpu_neck_regimes.py (the radix passes
restated, the union's scene kinds, the score lookup's queries, the key-range rows).  A plain module: no tests, no marks."""
import copy
import functools

import numpy as np
import torch

from proxytransformation_amd import MinkNeck, neck_host, sparse
from proxytransformation_amd.backbone import SparseLevel
from tests import sparse_util as su

NECK_ENTRY_POINTS = ("ptx_sparse_conv3d_act", "ptx_sparse_conv_transpose_gen", "ptx_neck_workspace_bytes", "ptx_neck_union_add",
                     "ptx_neck_prune_scores", "ptx_neck_topk_prune", "ptx_neck_head")
WIDTHS, OUT, K_PRUNE = (128, 256, 512, 1024), 256, 150
NEAR_TIE = 1e-5                    # of max |score| of the step: where fp32 and float64 may order two rows differently


def children(parents, ts):
    """The 8 children (tensor stride ts) of rows of tensor stride 2 ts, in the generative convolution's order."""
    c = np.repeat(np.asarray(parents, np.int64), 8, axis=0)
    c[:, 1:] += np.tile(sparse.kernel_offsets(2, ts), (len(parents), 1))
    return c.astype(np.int32)


@functools.lru_cache(maxsize=None)
def union_case():
    """``A = su.rows(4)``; ``B`` = the children of ~40 % of A's coarsened rows plus those of 30 parents (10 per non-empty scene) that
    coarsen no row of A -- rows in both, only in A and only in B, the empty and the one-row scene included.  Returns
    ``(a_coords, a_ends, b_coords, b_ends)``."""
    a, a_ends = su.rows(4)
    rng = np.random.default_rng(77)
    par, p_ends, _ = sparse.kernel_map_host(a, list(a_ends), 4, 1, 2)
    have = {tuple(r) for r in par.tolist()}
    rows, ends, lo = [], [], 0
    for b, hi in enumerate(p_ends):
        p = par[lo:hi]
        pick = p[np.sort(rng.permutation(len(p))[:int(round(0.4 * len(p)))])] if len(p) > 1 else p
        extra = []
        while len(p) and len(extra) < 10:
            cand = (b, *(int(v) * 8 for v in rng.integers(-60, 60, 3)))
            if cand not in have and cand not in extra:
                extra.append(cand)
        mix = np.concatenate([pick, np.asarray(extra, np.int32).reshape(-1, 4)])
        mix = mix[rng.permutation(len(mix))]
        rows.append(children(mix, 4))
        ends.append((ends[-1] if ends else 0) + 8 * len(mix))
        lo = hi
    return a, list(a_ends), np.concatenate(rows).astype(np.int32), ends


@functools.lru_cache(maxsize=None)
def e2e_levels(seed=5):
    """Four levels (tensor strides 8, 16, 32, 64) in three scenes -- 1500 and 600 random rows of stride 8 in [-16, 16)^3 * 8 and a
    single row -- each coarsened from the one before; features N(0, 1) of the shipped widths.  numpy arrays."""
    rng = np.random.default_rng(seed)
    cells = np.stack(np.meshgrid(*[np.arange(-16, 16)] * 3, indexing="ij"), -1).reshape(-1, 3)
    rows, ends = [], []
    for b, n in enumerate((1500, 600, 1)):
        pick = cells[rng.permutation(len(cells))[:n]] * 8
        rows.append(np.concatenate([np.full((n, 1), b), pick], 1))
        ends.append((ends[-1] if ends else 0) + n)
    c, ts = np.concatenate(rows).astype(np.int32), 8
    levels = []
    for w in WIDTHS:
        levels.append(SparseLevel(feats=rng.standard_normal((c.shape[0], w)).astype(np.float32), coords=c, scene_rows=list(ends),
                                  tensor_stride=ts))
        c, ends, _ = sparse.kernel_map_host(c, ends, ts, 1, 2)
        ts *= 2
    assert [lv.tensor_stride for lv in levels] == [8, 16, 32, 64] and levels[0].coords.shape[0] == 2101
    return levels


@functools.lru_cache(maxsize=None)
def e2e_neck(seed=6):
    """The shipped configuration in eval mode with random BatchNorm statistics (``su.bn_pair``'s draws), kaiming kernels scaled to keep the
    activations O(1), ``conv_cls.kernel ~ N(0, 1) / 16`` and bias -0.5: real scores are mostly negative, so the zero score of a row without
    a present corner matters."""
    torch.manual_seed(seed)
    m = MinkNeck(1, list(WIDTHS), OUT, 0.01, K_PRUNE)
    n = 0
    for mod in m.modules():
        if isinstance(mod, sparse.SparseBatchNorm):
            n += 1
            rng, C = np.random.default_rng(100 + n), mod.bn.num_features       # su.bn_pair's draws (which itself needs a device)
            with torch.no_grad():
                mod.bn.weight.copy_(torch.from_numpy(rng.uniform(0.5, 1.5, C).astype(np.float32)))
                mod.bn.bias.copy_(torch.from_numpy((rng.standard_normal(C) * 0.5).astype(np.float32)))
                mod.bn.running_mean.copy_(torch.from_numpy((rng.standard_normal(C) * 0.1).astype(np.float32)))
                mod.bn.running_var.copy_(torch.from_numpy(rng.uniform(0.5, 1.5, C).astype(np.float32)))
    with torch.no_grad():
        for name, p in m.named_parameters():
            if name.endswith("kernel") and not name.startswith("conv_cls"):
                p.normal_(0.0, (1.0 / (p.shape[1] * (1 if p.shape[0] == 8 else 9))) ** 0.5)
        m.conv_cls.kernel.copy_(torch.randn(1, OUT, 1) / 16)
        m.conv_cls.bias.fill_(-0.5)
    return m.eval()


def near_ties(scores, scene_rows, k):
    """Per scene with more than k rows: how many rows lie within ``NEAR_TIE * max |scores|`` of the scene's k-th largest score WITHOUT
    being equal to it.  Equal scores (the exact 0.0 of rows without a present corner, above all) are no near-ties: both sides decide them
    by the row index; a near-tie is a pair that two precisions may order differently.  ``[(scene, count, k-th score)]``."""
    s = np.asarray(scores, np.float64).reshape(-1)
    margin = NEAR_TIE * float(np.abs(s).max()) if s.size else 0.0
    out, lo = [], 0
    for b, hi in enumerate(int(e) for e in scene_rows):
        if hi - lo > k:
            kth = np.sort(s[lo:hi])[::-1][k - 1]
            d = np.abs(s[lo:hi] - kth)
            out.append((b, int(((d <= margin) & (d > 0)).sum()), float(kth)))
        lo = hi
    return out


def bits(got, ref: np.ndarray):
    """``got`` (a device tensor or an array) equals ``ref`` in shape, dtype and every bit."""
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    assert got.shape == ref.shape and got.dtype == ref.dtype, (got.shape, ref.shape, got.dtype, ref.dtype)
    assert np.array_equal(got.view(np.uint32) if got.dtype == np.float32 else got, ref.view(np.uint32) if ref.dtype == np.float32 else ref)


def end_to_end(levels, m, batch, k):
    """The end-to-end protocol: (a) ``forward`` against ``forward_host(keep=the device's masks)``: row sets, order and points bit for
    bit, feats and scores by ``hold``; (b) per pruning step the device's mask and the host's own float64 mask differ only on rows within
    ``NEAR_TIE * max |score|`` of the step's k-th score, and on no more rows than that step and scene has near-ties (``near_ties``, which
    the host test caps at 2 % of k).  Returns the host's trace."""
    dev_levels = [SparseLevel(su.dev(lv.feats), su.dev(lv.coords), lv.scene_rows, lv.tensor_stride) for lv in levels]
    gm = copy.deepcopy(m).to(su.DEV)
    keep = []
    with torch.no_grad():
        feats, scores, points = gm(dev_levels, batch, keep_out=keep)
    masks = [k_.cpu().numpy() for k_ in keep]
    trace = []
    f64, s64, p64 = m.forward_host(levels, batch, np.float64, keep=masks, trace=trace)
    f32, s32, _ = m.forward_host(levels, batch, np.float32, keep=masks)
    assert len(masks) == 3 and len(feats) == batch
    for b in range(batch):
        bits(points[b], p64[b])
        assert feats[b].shape == f64[b].shape and scores[b].shape == s64[b].shape == (f64[b].shape[0], m.num_classes)
    cat = lambda parts: np.concatenate([np.asarray(p.cpu() if isinstance(p, torch.Tensor) else p) for p in parts])      # noqa: E731
    su.hold("neck feats", cat(feats), cat(f32), cat(f64))
    su.hold("neck scores", cat(scores), cat(s32), cat(s64))
    for step, (mask, tr) in enumerate(zip(masks, trace)):
        s = tr["scores"]
        margin = NEAR_TIE * float(np.abs(s).max())
        differ = np.nonzero(mask != tr["keep"])[0]
        ties = {scene: count for scene, count, _ in near_ties(s, tr["scene_rows"], k)}
        lo = 0
        for scene, hi in enumerate(tr["scene_rows"]):
            if hi - lo > k:
                kth = np.sort(s[lo:hi])[::-1][k - 1]
                d = differ[(differ >= lo) & (differ < hi)]
                print(f"step {step} scene {scene}: {len(d)} rows differ, k-th score {kth:+.4f}")
                assert (np.abs(s[d] - kth) <= margin).all() and len(d) <= ties[scene] <= 0.02 * k
            else:
                assert not ((differ >= lo) & (differ < hi)).any()
            lo = hi
    return trace


# ------------------------------------------------------------------------------------------------------------------ second end-to-end configuration
CLASSES_B, K_PRUNE_B = 3, 520      # 520: the 40-row scene reaches 8^3 = 512 rows at the last step and is never pruned


@functools.lru_cache(maxsize=None)
def e2e_levels_b(seed=21):
    """Four levels (tensor strides 8 to 64) in four scenes: 1500 rows of stride 8 in [-8, 8)^3 * 8 (8 rows at stride 64; 64, 512 and 4096
    rows before the three prunes: pruned at the last step only), no row, 40 rows inside one stride-64 voxel (8, 64, 512 rows: never
    pruned at k = 520), 600 rows in [-16, 16)^3 * 8 (64 rows at stride 64, 512 before the first prune: not pruned there, pruned at the
    two later steps)."""
    rng = np.random.default_rng(seed)

    def cells(lo, hi):
        return np.stack(np.meshgrid(*[np.arange(lo, hi)] * 3, indexing="ij"), -1).reshape(-1, 3)

    rows, ends = [], []
    for b, (n, c) in enumerate(((1500, cells(-8, 8)), (0, cells(0, 1)), (40, cells(8, 16)), (600, cells(-16, 16)))):
        pick = c[rng.permutation(len(c))[:n]] * 8
        rows.append(np.concatenate([np.full((n, 1), b), pick], 1))
        ends.append((ends[-1] if ends else 0) + n)
    c, ts = np.concatenate(rows).astype(np.int32), 8
    levels = []
    for w in WIDTHS:
        levels.append(SparseLevel(feats=rng.standard_normal((c.shape[0], w)).astype(np.float32), coords=c, scene_rows=list(ends),
                                  tensor_stride=ts))
        c, ends, _ = sparse.kernel_map_host(c, ends, ts, 1, 2)
        ts *= 2
    top = levels[3].scene_rows
    assert levels[0].scene_rows == [1500, 1500, 1540, 2140] and top[1] == top[0] and top[2] - top[1] == 1 and top[0] == 8 and top[3] - top[2] == 64
    return levels


@functools.lru_cache(maxsize=None)
def e2e_neck_b(seed=22):
    """``e2e_neck`` with three classes (``conv_cls.kernel ~ N(0, 1) / 16``, bias -0.5) and ``pts_prune_threshold = 520``."""
    torch.manual_seed(seed)
    b = MinkNeck(CLASSES_B, list(WIDTHS), OUT, 0.01, K_PRUNE_B)
    b.load_state_dict({k: v for k, v in e2e_neck().state_dict().items() if not k.startswith("conv_cls")}, strict=False)
    with torch.no_grad():
        b.conv_cls.kernel.copy_(torch.randn(1, OUT, CLASSES_B) / 16)
        b.conv_cls.bias.fill_(-0.5)
    return b.eval()


# ------------------------------------------------------------------------------------------------------------------ top-k
def radix_trace(scores, lo, hi, k):
    """The four 8-bit passes of topk_threshold (csrc/head.h) over ``topk_key(scores[lo:hi])`` restated: per pass (shift 24, 16, 8, 0)
    ``(occupied digits among the candidates, need behind the pass)``; then the threshold key.  ``need``: rows still to take among those
    that match the prefix."""
    key = neck_host.topk_key(np.asarray(scores, np.float32)[lo:hi]).astype(np.uint64)
    assert hi - lo > k >= 1
    prefix, known, need, passes = 0, 0, int(k), []
    for shift in (24, 16, 8, 0):
        cand = key[(key & np.uint64(known)) == np.uint64(prefix)]
        hist = np.bincount(((cand >> np.uint64(shift)) & np.uint64(255)).astype(np.int64), minlength=256)
        d = 255
        while d > 0 and hist[d] < need:
            need -= int(hist[d])
            d -= 1
        prefix |= d << shift
        known |= 255 << shift
        passes.append((int((hist > 0).sum()), need))
    return passes, prefix


LOW_BYTE_ROWS, LOW_BYTE_K = 5000, (1, 255, 256, 257, 2500, 4999)


@functools.lru_cache(maxsize=None)
def low_byte_scores(kind):
    """5000 scores that differ in their low 16 bits only: bit patterns ``0x3F000000 + U[0, 2^16)`` (``positive``), ``0xBF000000 + ...``
    (``negative``: the inverted-key branch), half of each (``mixed``); ``normal``: N(0, 1), which splits in the first two passes."""
    rng = np.random.default_rng(31)
    low = rng.integers(0, 1 << 16, LOW_BYTE_ROWS).astype(np.uint32)
    if kind == "normal":
        return rng.standard_normal(LOW_BYTE_ROWS).astype(np.float32)
    top = {"positive": np.full(LOW_BYTE_ROWS, 0x3F000000, np.uint32), "negative": np.full(LOW_BYTE_ROWS, 0xBF000000, np.uint32),
           "mixed": np.where(rng.permutation(LOW_BYTE_ROWS) % 2 == 0, 0x3F000000, 0xBF000000).astype(np.uint32)}[kind]
    return (top + low).view(np.float32)


def check_low_byte_passes(kind):
    """The condition that makes the low-byte case mean something: at every k the passes at shift 8 and shift 0 each see at least two
    occupied digits among their candidates (``normal``: the passes at shift 24 and 16)."""
    s = low_byte_scores(kind)
    for k in LOW_BYTE_K:
        passes, prefix = radix_trace(s, 0, len(s), k)
        want = (0, 1) if kind == "normal" else (2, 3)
        assert all(passes[p][0] >= 2 for p in want), (kind, k, passes)
        assert prefix == int(np.sort(neck_host.topk_key(s))[::-1][k - 1]) and passes[3][1] >= 1, (kind, k)
    if kind != "normal":
        assert len(np.unique(s)) > 4000 and (np.signbit(s).all() if kind == "negative" else np.signbit(s).any() == (kind == "mixed"))


TOPK_64_SIZES, TOPK_64_K = [0, 1, 99, 100, 101, 255, 256, 257, 300], 100


def scene_rows_of(sizes):
    """Rows ``(scene, i, -i, 7)`` and the scene ends of scenes of the given sizes: coordinates that name their row."""
    rows = np.concatenate([np.stack([np.full(n, b), np.arange(n), -np.arange(n), np.full(n, 7)], 1) for b, n in enumerate(sizes)])
    return rows.astype(np.int32), np.cumsum(sizes).tolist()


@functools.lru_cache(maxsize=None)
def special_scores():
    """28 scores in a fixed shuffle, by descending key: 2 positive NaNs (one quiet, one with payload 1), 2 +inf, 5 positive finite, 3
    positive denormals, 4 zeros of both signs, 3 negative denormals, 5 negative finite, 2 -inf, 2 negative NaNs -- and the k that put the
    threshold on +inf (just below the positive NaNs; one of two kept), a positive denormal, the zero key (two of four kept), a negative
    denormal, -inf (one of two kept).  Assembled as bit patterns: no conversion touches a payload."""
    f = lambda *v: np.array(v, np.float32).view(np.uint32)   # noqa: E731
    den = np.array([1, 0x1234, 0x7FFFFF], np.uint32)
    u = np.concatenate([np.array([0x7FC00000, 0x7F800001], np.uint32), f(np.inf, np.inf), f(3.5, 1.0, 0.25, 1e-30, 2e-38), den,
                        f(0.0, -0.0, 0.0, -0.0), den | np.uint32(1 << 31), f(-2e-38, -1e-30, -0.25, -1.0, -3.5), f(-np.inf, -np.inf),
                        np.array([0xFFC00000, 0xFF800001], np.uint32)])
    assert u.dtype == np.uint32 and len(u) == 28 and u[9] == 1 and u[12] == 0 and u[13] == 1 << 31
    order = np.random.default_rng(32).permutation(len(u))
    return u[order].view(np.float32), {"+inf": 3, "+denormal": 11, "zero": 14, "-denormal": 18, "-inf": 25}


# ------------------------------------------------------------------------------------------------------------------ union
UNION_KINDS = ("both empty", "A only", "B only", "disjoint", "B in A", "A in B", "mixed")
M_VOX, m_VOX = (1 << 18) - 1, -(1 << 18)     # the last and the first voxel of the key range, in tensor strides


@functools.lru_cache(maxsize=None)
def union_regime_case():
    """64 scenes at tensor stride 4 cycling through ``UNION_KINDS``; ``mixed``: A = 400 shared + 50 own rows, B = the 400 shared + 420 own
    rows in random order (820 rows: four 256-row runs).  ``(a_coords, a_ends, b_coords, b_ends)``; more rows in B than in A."""
    rng = np.random.default_rng(41)
    cells = np.stack(np.meshgrid(*[np.arange(-12, 12)] * 3, indexing="ij"), -1).reshape(-1, 3) * 4
    a_rows, b_rows, a_ends, b_ends = [], [], [], []
    for b in range(64):
        c = cells[rng.permutation(len(cells))]
        na, nb, both = [(0, 0, 0), (40, 0, 0), (0, 50, 0), (30, 45, 0), (60, 25, 25), (20, 70, 20), (450, 820, 400)][b % 7]
        a = c[:na]                                              # the shared rows: the first `both` of A
        bb = np.concatenate([c[:both], c[na:na + nb - both]])
        bb = bb[rng.permutation(len(bb))]
        a = a[rng.permutation(len(a))]
        a_rows.append(np.concatenate([np.full((na, 1), b), a], 1))
        b_rows.append(np.concatenate([np.full((nb, 1), b), bb], 1))
        a_ends.append((a_ends[-1] if a_ends else 0) + na)
        b_ends.append((b_ends[-1] if b_ends else 0) + nb)
    return np.concatenate(a_rows).astype(np.int32), a_ends, np.concatenate(b_rows).astype(np.int32), b_ends


def union_kinds(a, a_ends, b, b_ends):
    """The kind of every scene, from the rows themselves; a ``mixed`` scene must have >= 800 rows in B, 40 to 60 % of them unmatched,
    matched and unmatched rows in every 256-row run."""
    kinds, alo, blo = [], 0, 0
    for ahi, bhi in zip(a_ends, b_ends):
        sa = {tuple(r) for r in a[alo:ahi].tolist()}
        hit = np.array([tuple(r) in sa for r in b[blo:bhi].tolist()], bool)
        na, nb, both = ahi - alo, bhi - blo, int(hit.sum())
        if na == 0 or nb == 0:
            kind = ("both empty", "B only", "A only")[(nb > 0) + 2 * (na > 0)]
        elif both == 0:
            kind = "disjoint"
        elif both == nb and nb < na:
            kind = "B in A"
        elif both == na and na < nb:
            kind = "A in B"
        else:
            kind = "mixed"
            assert nb >= 800 and 0.4 < 1 - both / nb < 0.6 and both < na
            assert all(0 < hit[r:r + 256].sum() < len(hit[r:r + 256]) for r in range(0, nb, 256))
        kinds.append(kind)
        alo, blo = ahi, bhi
    return kinds


def union_key_range_case(a_outside=False):
    """Two scenes at tensor stride 4 with rows at the ends of the key range.  Scene 0: the pairs (0, 0, M) / (0, 1, m) and (0, M, 5) /
    (1, m, 5) of test_gpu_sparse_regimes -- a coordinate one past M would carry into the next field and alias the pair's other row --
    with (0, 0, M) and (0, M, 5) in both sets, (0, 1, m) in A only, (1, m, 5) in B only; B also holds (0, 0, 2^18), OUTSIDE the range and
    an alias of A's (0, 1, m): no row of A, so it is appended.  Scene 1: (m, 7, 7) in A, (M, M, M) in both, (m, m, m) in B.
    ``a_outside``: A's scene 1 also holds (2^18, 7, 7), which the call must refuse."""
    M, m = M_VOX, m_VOX
    a = [(0, 0, 0, M), (0, 0, 1, m), (0, 0, M, 5), (0, 3, 3, 3), (1, m, 7, 7), (1, M, M, M)] + ([(1, M + 1, 7, 7)] if a_outside else [])
    b = [(0, 0, M, 5), (0, 1, m, 5), (0, 0, 0, M + 1), (0, 0, 0, M), (1, M, M, M), (1, m, m, m)]
    scale = np.array([1, 4, 4, 4], np.int32)
    return np.array(a, np.int32) * scale, [4, len(a)], np.array(b, np.int32) * scale, [4, 6]


# ------------------------------------------------------------------------------------------------------------------ score lookup
def corner_table(q, s_coords, s_rows, ts):
    """``(n_q, 8)`` row index of every corner of every query in ``prune_scores_host``'s order, -1 where absent."""
    index, lo = {}, 0
    for b, hi in enumerate(int(e) for e in s_rows):
        for i in range(lo, hi):
            index[(b, *(int(v) for v in s_coords[i, 1:]))] = i
        lo = hi
    offs = sparse.kernel_offsets(2, ts)
    out = np.full((len(q), 8), -1, np.int64)
    for i, row in enumerate(np.asarray(q, np.int64)):
        l = np.floor_divide(row[1:], ts) * ts
        for j, d in enumerate(offs):
            out[i, j] = index.get((int(row[0]), *(int(v) for v in l + d)), -1)
    return out


def corner_weights(q, ts):
    """``(n_q, 8, 3)`` float32: the per-axis factors ``1 - |q - c| / ts`` of every corner, exact in fp32."""
    q = np.asarray(q, np.int64)[:, 1:]
    l = np.floor_divide(q, ts) * ts
    c = l[:, None, :] + sparse.kernel_offsets(2, ts)[None]
    return (np.float32(1) - np.abs(q[:, None, :] - c).astype(np.float32) * (np.float32(1) / np.float32(ts))).astype(np.float32)


@functools.lru_cache(maxsize=None)
def score_query_case(ts):
    """Score rows ``su.rows(ts)`` (a dense block, a sparse random scene, an empty scene, a one-row scene), N(0, 1) scores and ~3300 queries
    at arbitrary integer coordinates: uniform in and around the block, a score row plus an offset in (-ts, ts)^3 in the other scenes (so
    negative coordinates off the lattice occur), 100 in the scene without score rows.  ``(q, s_coords, s_ends, scores)``."""
    s_coords, s_ends = su.rows(ts)
    s_ends = list(s_ends)
    rng = np.random.default_rng(51 + ts)
    scores = rng.standard_normal(len(s_coords)).astype(np.float32)
    q0 = np.concatenate([np.zeros((1300, 1), np.int64), rng.integers(-4 * ts, 4 * ts, (1300, 3))], 1)
    base = s_coords[s_ends[0]:s_ends[1]][rng.integers(0, s_ends[1] - s_ends[0], 1800)].astype(np.int64)
    base[:, 1:] += rng.integers(-ts + 1, ts, (1800, 3))
    q2 = np.concatenate([np.full((100, 1), 2), rng.integers(-4 * ts, 4 * ts, (100, 3))], 1)
    q3 = np.repeat(s_coords[s_ends[2]:s_ends[3]].astype(np.int64), 100, axis=0)
    q3[:, 1:] += rng.integers(-ts - 1, ts + 2, (100, 3))
    return np.concatenate([q0, base, q2, q3]).astype(np.int32), s_coords, s_ends, scores


def check_score_query_case(ts):
    """The preconditions of the inexact case: >= 3000 queries, negative coordinates off the lattice, queries with 0, 1, 2, 4 and 8 present
    corners, and more than half of the present ``(w, s)`` pairs with an inexact fp32 product ``w * s`` (decided through float64, which
    holds the product of two fp32 numbers exactly).  ``ts`` > 4096 (factors of more than 12 bits): the product of two factors is rounded too, and for
    more than a quarter of the present corners (over a thousand) the product in the order z, y, x differs from ``(x * y) * z``."""
    q, s_coords, s_ends, scores = score_query_case(ts)
    corners = corner_table(q, s_coords, s_ends, ts)
    present = corners >= 0
    count = present.sum(1)
    assert len(q) >= 3000 and ((q[:, 1:] < 0) & (q[:, 1:] % ts != 0)).any(axis=1).sum() > 500
    assert {0, 1, 2, 4, 8} <= set(count.tolist()) and (count[q[:, 0] == 2] == 0).all()
    f = corner_weights(q, ts)
    w = (f[..., 0] * f[..., 1]) * f[..., 2]
    prod = w.astype(np.float64)[present] * scores[corners[present]].astype(np.float64)
    assert float((prod.astype(np.float32).astype(np.float64) != prod).mean()) > 0.5
    exact = f.astype(np.float64).prod(axis=2)
    if ts <= 256:
        assert np.array_equal(w.astype(np.float64), exact)
    else:
        assert ts > 4096 and float((w != (f[..., 2] * f[..., 1]) * f[..., 0])[present].mean()) > 0.25
    return corners


def score_edge_case(axis):
    """Tensor stride 4, two scenes.  The query sits inside the last voxel M of ``axis`` (one off the lattice), so its +1 corners on that
    axis are at 2^18, outside the key range; the row that coordinate would alias by carrying into the next field -- the next y, the
    next x, the next scene, at the first voxel m -- is a score row with score 1e6.  ``(q, s_coords, s_ends, scores)``."""
    M, m = M_VOX, m_VOX
    here, alias = {2: ((0, 0, 0, M), (0, 0, 1, m)), 1: ((0, 0, M, 5), (0, 1, m, 5)), 0: ((0, M, 7, 7), (1, m, 7, 7))}[axis]
    near = list(here)
    near[1 + (axis + 1) % 3] += 1                            # a second present corner of the query
    rows = sorted({here, tuple(near), alias, (1, 2, 2, 2)})
    s_coords = np.array(rows, np.int32) * np.array([1, 4, 4, 4], np.int32)
    s_ends = [sum(r[0] == 0 for r in rows), len(rows)]
    scores = np.array([1e6 if r == alias else 1.5 + i for i, r in enumerate(rows)], np.float32)
    q = np.array([here, here], np.int32) * np.array([1, 4, 4, 4], np.int32)
    q[0, 1:] += 1                                            # inside the voxel on every axis
    q[1, 1 + axis] += 3
    return q, s_coords, s_ends, scores


@functools.lru_cache(maxsize=None)
def score_64_case():
    """64 scenes at tensor stride 2 with 0, 1, 30 and 200 score rows in turn; 20 queries per scene: around its rows, or (the 16 scenes
    without score rows) around the origin."""
    rng = np.random.default_rng(61)
    cells = np.stack(np.meshgrid(*[np.arange(-5, 5)] * 3, indexing="ij"), -1).reshape(-1, 3) * 2
    rows, ends, qs = [], [], []
    for b in range(64):
        n = (0, 1, 30, 200)[b % 4]
        c = cells[rng.permutation(len(cells))[:n]]
        rows.append(np.concatenate([np.full((n, 1), b), c], 1))
        ends.append((ends[-1] if ends else 0) + n)
        base = c[rng.integers(0, n, 20)] if n else np.zeros((20, 3), np.int64)
        qs.append(np.concatenate([np.full((20, 1), b), base + rng.integers(-1, 2, (20, 3))], 1))
    return np.concatenate(qs).astype(np.int32), np.concatenate(rows).astype(np.int32), ends, rng.standard_normal(ends[-1]).astype(np.float32)
