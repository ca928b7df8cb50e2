#!/usr/bin/env python3
"""Time the eval forward of the shipped ``MinkNeck`` ([128, 256, 512, 1024] -> 256, one class, pts_prune_threshold 1000) on an MI355X and
write the report profiles/mink_neck.txt keeps.

Input: six room clouds of 100 000 points quantised at 1 cm through ``MinkResNet(34, 3)`` (the input of profiles/sparse_norm.txt); every
level's features are concatenated with as many random channels (the place of the sampled image features; the caller concatenates).

Two sides, whole calls through Python (wrappers, ctypes, ``torch.empty`` of the outputs, the host waits for row counts), HIP events:

* the neck's stages one by one, each on the HIP chain's own inputs of that stage -- generative transposed convolution, its 3x3x3
  convolution (+ kernel map), union add, prune scores, top-k prune, the output block (+ kernel map), the head -- summed over the levels;
* the torch composition of the same stage on the same rows, as a user could write it today: ``mm`` per offset (given OUR neighbour table
  as per-offset index lists made outside the timing: ``index_select`` + ``mm`` + ``index_add_``), sorted int64 keys + ``searchsorted`` for
  the union and the corner lookup, ``torch.topk`` per scene and boolean indexing.  The kernel maps are counted on the HIP side only (the
  torch side has no substitute for them and is handed the table).

Per stage and side: the median of --blocks blocks of --reps calls after a warm-up block, the sides alternating.  Then the whole
``forward`` (median of --blocks calls), which is what a user pays.

Usage (on a GPU):  python tools/mink_neck_time.py [--blocks 5] [--reps 4] [--out profiles/mink_neck.txt]
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from sparse_conv_time import B, N, VOXEL, alternate, offset_lists, room_points, torch_layer      # noqa: E402

WIDTHS, OUT, K = (128, 256, 512, 1024), 256, 1000


def keys(c):
    """(scene, x, y, z) int32 rows -> one int64 per row (coordinates within +-2^19)."""
    c = c.long()
    return (c[:, 0] << 60) | ((c[:, 1] + (1 << 19)) << 40) | ((c[:, 2] + (1 << 19)) << 20) | (c[:, 3] + (1 << 19))


def lookup(table_keys, order, q):
    """Row of each key of q in the table (sorted keys + the permutation that sorted them), -1 where absent."""
    pos = torch.searchsorted(table_keys, q).clamp(max=table_keys.numel() - 1)
    return torch.where(table_keys[pos] == q, order[pos], torch.full_like(pos, -1))


def t_gen(c, x, kernel, scale, shift, half):
    out = F.elu(torch.stack([x @ kernel[j] for j in range(8)], 1).reshape(-1, kernel.shape[2]) * scale + shift)
    offs = torch.tensor([[0, j & 1, (j >> 1) & 1, j >> 2] for j in range(8)], dtype=torch.int32, device=c.device) * half
    return (c[:, None, :] + offs[None]).reshape(-1, 4), out


def t_conv(x, lists, n_out, weight, scale, shift):
    return F.elu(torch_layer(x, weight, lists, n_out) * scale + shift)


def t_union(ac, a_ends, af, bc, b_ends, bf):
    ka, order = torch.sort(keys(ac))
    hit = lookup(ka, order, keys(bc))
    f = af.clone()
    m = hit >= 0
    f.index_add_(0, hit[m], bf[m])
    cs, fs, alo, blo = [], [], 0, 0
    for ahi, bhi in zip(a_ends, b_ends):
        alone = ~m[blo:bhi]
        cs += [ac[alo:ahi], bc[blo:bhi][alone]]
        fs += [f[alo:ahi], bf[blo:bhi][alone]]
        alo, blo = ahi, bhi
    return torch.cat(cs), torch.cat(fs)


def t_scores(q, sc, s, ts):
    ks, order = torch.sort(keys(sc))
    low = torch.div(q[:, 1:], ts, rounding_mode="floor") * ts
    acc = torch.zeros(q.shape[0], dtype=torch.float32, device=q.device)
    for j in range(8):
        d = torch.tensor([j & 1, (j >> 1) & 1, j >> 2], dtype=q.dtype, device=q.device) * ts
        corner = torch.cat([q[:, :1], low + d], 1)
        row = lookup(ks, order, keys(corner))
        w = (1 - (q[:, 1:] - corner[:, 1:]).abs().float() / ts).prod(1)
        acc = acc + torch.where(row >= 0, w * s[row.clamp(min=0)], torch.zeros_like(w))
    return acc


def t_topk(score, c, ends, f, k):
    mask = torch.zeros_like(score, dtype=torch.bool)
    lo = 0
    for hi in ends:
        if hi > lo:
            mask[lo + torch.topk(score[lo:hi], min(hi - lo, k), sorted=False).indices] = True
        lo = hi
    return c[mask], f[mask]


def t_head(x, w, b):
    cls = x @ w + b
    return cls, cls.max(1).values


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mink_neck.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mink_neck_time.py measures on a GPU: none found")
    from bench import build_module
    from proxytransformation_amd import MinkNeck, MinkResNet, neck, sparse
    from proxytransformation_amd.backbone import SparseLevel
    from proxytransformation_amd.synth import CONFIGS
    dev = torch.device("cuda:0")
    mod, _ = build_module(CONFIGS["cfg4_room"], dev)
    torch.manual_seed(0)
    net = MinkResNet(34, 3).to(dev).eval()
    m = MinkNeck(1, list(WIDTHS), OUT, VOXEL, K).to(dev).eval()
    m.init_weights()
    gen = torch.Generator(device=dev).manual_seed(3)
    stages = ["generative conv", "map + conv k3 (up)", "union add", "prune scores", "top-k prune", "map + conv k3 (out)", "head"]
    hip = {k: 0.0 for k in stages}
    tor = {k: 0.0 for k in stages}
    diff = {k: 0.0 for k in stages}
    lines = []
    with torch.no_grad():
        pts = [torch.from_numpy(room_points(900 + b, N)).to(dev) for b in range(B)]
        coords, feats3, ends = mod.quantize(pts, VOXEL, return_scene_rows=True)
        levels = [SparseLevel(torch.cat([lv.feats, torch.randn(lv.feats.shape, generator=gen, device=dev)], 1).contiguous(), lv.coords,
                              lv.scene_rows, lv.tensor_stride) for lv in net(coords, ends, feats3.contiguous())]

        def both(name, hip_fn, torch_fn):
            med, _, last = alternate({"hip": hip_fn, "torch": torch_fn}, args.blocks, args.reps)
            hip[name] += med["hip"]
            tor[name] += med["torch"]
            flo = lambda r: [t for t in (r if isinstance(r, tuple) else (r,)) if isinstance(t, torch.Tensor) and t.is_floating_point()]  # noqa: E731
            for h, t in zip(flo(last["hip"]), flo(last["torch"])):       # the two sides agree (the top-k may break ties differently)
                if h.shape == t.reshape(h.shape if h.numel() == t.numel() else t.shape).shape and h.numel():
                    diff[name] = max(diff[name], float((h - t.reshape(h.shape)).abs().max() / t.abs().max().clamp(min=1e-30)))
                else:
                    diff[name] = float("nan")
            return last["hip"]

        top = len(levels) - 1
        c, e, ts, x = levels[top].coords, list(levels[top].scene_rows), levels[top].tensor_stride, levels[top].feats
        score = None
        rows = []
        for i in range(top, -1, -1):
            if i < top:
                up = getattr(m, f"up_block_{i + 1}")
                s0, h0 = sparse.bn_fold(up[1].bn)
                gc, ge, g = both(stages[0], lambda: up[0](c, e, ts, x, scale=s0, shift=h0, act=2), lambda: t_gen(c, x, up[0].kernel, s0, h0, ts // 2))
                s1, h1 = sparse.bn_fold(up[4].bn)
                lists = offset_lists(sparse.kernel_map(gc, ge, ts // 2, 3, 1).nbr)
                g2 = both(stages[1], lambda: up[3](g, sparse.kernel_map(gc, ge, ts // 2, 3, 1), scale=s1, shift=h1, elu=True),
                          lambda: t_conv(g, lists, gc.shape[0], up[3].kernel, s1, h1))
                lv = levels[i]
                uc, ue, u = both(stages[2], lambda: neck.union_add(lv.coords, lv.scene_rows, lv.feats, gc, ge, g2, ts // 2),
                                 lambda: t_union(lv.coords, lv.scene_rows, lv.feats, gc, ge, g2))
                q = both(stages[3], lambda: neck.prune_scores(uc, c, e, ts, score), lambda: t_scores(uc, c, score, ts))
                rows.append((int(gc.shape[0]), int(uc.shape[0])))
                c, e, x, _ = both(stages[4], lambda: neck.topk_prune(q, uc, ue, u, K), lambda: t_topk(q, uc, ue, u, K))
                ts //= 2
            ob = getattr(m, f"out_block_{i}")
            so, ho = sparse.bn_fold(ob[1].bn)
            lists = offset_lists(sparse.kernel_map(c, e, ts, 3, 1).nbr)
            out = both(stages[5], lambda: ob[0](x, sparse.kernel_map(c, e, ts, 3, 1), scale=so, shift=ho, elu=True),
                       lambda: t_conv(x, lists, c.shape[0], ob[0].kernel, so, ho))
            w, bias = m.conv_cls.kernel[0], m.conv_cls.bias
            _, score = both(stages[6], lambda: neck.neck_head(out, m.conv_cls.kernel, m.conv_cls.bias), lambda: t_head(out, w, bias))
        total = []
        for blk in range(args.blocks + 1):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            feats, scores, points = m(levels, B)
            b.record()
            b.synchronize()
            if blk:
                total.append(a.elapsed_time(b))
    lines.append(f"MinkNeck({list(WIDTHS)} -> {OUT}, 1 class, pts_prune_threshold {K}) eval forward; {torch.cuda.get_device_name(0)}; {B} room "
                 f"clouds x {N} points at {VOXEL * 100:g} cm -> levels of {[int(lv.feats.shape[0]) for lv in levels]} rows; per step (generated rows, "
                 f"union rows): {rows}; output rows per scene: {[int(f.shape[0]) for f in feats]}")
    lines.append(f"per stage, summed over the levels, median of {args.blocks} blocks of {args.reps} calls, sides alternating; whole calls through "
                 f"Python; the torch side is handed the neighbour tables (kernel maps are on the HIP side only)")
    for k in stages:
        lines.append(f"  {k:22s} hip {hip[k]:9.1f} us   torch {tor[k]:9.1f} us   torch / hip {tor[k] / hip[k]:5.2f}" +
                     f"   max |hip - torch| / max |torch| {diff[k]:.1e}" + ("   SLOWER than the torch composition" if hip[k] > tor[k] else ""))
    lines.append(f"  {'sum of the stages':22s} hip {sum(hip.values()):9.1f} us   torch {sum(tor.values()):9.1f} us   torch / hip "
                 f"{sum(tor.values()) / sum(hip.values()):5.2f}")
    lines.append(f"whole forward (one call, median of {args.blocks}): {statistics.median(total):.3f} ms (min {min(total):.3f}, max {max(total):.3f})")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
