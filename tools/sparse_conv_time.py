#!/usr/bin/env python3
"""Time the sparse convolution on the voxel rows (proxytransformation_amd/sparse.py: ptx_sparse_kernel_map + ptx_sparse_conv3d) and
write the report profiles/sparse_conv.txt keeps.

Input: six room clouds of 100 000 points (the surfaces of a 7 x 5 x 3 m room) through ``quantize`` at 1 cm, and the levels
``pipeline.level_coordinates`` makes of them.  Three layers of a MinkResNet (backbones/mink_resnet.py):
  stem      kernel map (k3, stride 2) of the 1 cm rows + the 3 -> 64 convolution      (map and convolution timed apart and together)
  64x64     a 64 -> 64 k3 stride-1 layer on the rows of tensor stride 8               (the map is built once, outside the timing)
  512x512   a 512 -> 512 k3 stride-1 layer on the rows of tensor stride 64
Baseline: the torch composition a user could write today GIVEN our neighbour table -- per offset ``index_select`` + ``mm`` +
``index_add_`` (27 triples; the per-offset index lists are made from the table once, outside the timing).  Same GPU, HIP events around
blocks of --reps calls, the two sides alternating from block to block, reported = median of the blocks.  Besides the ratio: the
convolution's share of the fp32 matrix peak (157 TF) from 2 * (present neighbours) * Cin * Cout FLOP, and of HBM (8 TB/s) from the
gathered bytes (present neighbours * Cin * 4) plus the output.

``--pairs LOG``: copy the accuracy pairs tests/test_gpu_sparse_conv.py prints (lines starting with "sparse_conv ") into the report.

Usage (on a GPU):  python tools/sparse_conv_time.py [--blocks 7] [--reps 20] [--pairs pytest.log] [--out profiles/sparse_conv.txt]
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
B, N, VOXEL = 6, 100000, 0.01
PEAK_TF, PEAK_TBS = 157.0, 8.0


def room_points(seed, n, extent=(7.0, 5.0, 3.0)):
    """n points on the six faces of a box-shaped room (area-weighted), 2 mm of noise off the surface."""
    rng = np.random.default_rng(seed)
    ex = np.asarray(extent)
    area = np.array([ex[1] * ex[2], ex[1] * ex[2], ex[0] * ex[2], ex[0] * ex[2], ex[0] * ex[1], ex[0] * ex[1]])
    face = rng.choice(6, size=n, p=area / area.sum())
    p = rng.random((n, 3)) * ex
    axis, side = face // 2, face % 2
    p[np.arange(n), axis] = side * ex[axis] + rng.normal(0.0, 0.002, n)
    return p.astype(np.float32)


def block_us(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        r = fn()
    b.record()
    b.synchronize()
    return 1e3 * a.elapsed_time(b) / reps, r


def alternate(sides, blocks, reps):
    """{name: fn} -> ({name: median us}, {name: [block us]}, {name: last result}); block 0 warms up, the order flips per block."""
    names = list(sides)
    t = {k: [] for k in names}
    last = {}
    for blk in range(blocks + 1):
        for k in (names if blk % 2 == 0 else names[::-1]):
            us, last[k] = block_us(sides[k], reps)
            if blk:
                t[k].append(us)
    return {k: statistics.median(v) for k, v in t.items()}, t, last


def torch_layer(feats, weight, lists, n_out):
    """27 x (index_select, mm, index_add_): what a user writes today, given the neighbour table."""
    out = torch.zeros((n_out, weight.shape[2]), dtype=torch.float32, device=feats.device)
    for j, (src, dst) in enumerate(lists):
        if src.numel():
            out.index_add_(0, dst, feats.index_select(0, src) @ weight[j])
    return out


def offset_lists(nbr):
    lists = []
    for j in range(nbr.shape[1]):
        dst = torch.nonzero(nbr[:, j] >= 0).reshape(-1)
        lists.append((nbr[dst, j].long(), dst))
    return lists


def layer_report(name, feats, kmap, weight, blocks, reps, lines, map_fn=None):
    from proxytransformation_amd import sparse
    lists = offset_lists(kmap.nbr)
    n_out, kvol = kmap.nbr.shape
    present = int((kmap.nbr >= 0).sum())
    cin, cout = int(weight.shape[1]), int(weight.shape[2])
    sides = {"hip": lambda: sparse.sparse_conv3d(feats, kmap, weight), "torch": lambda: torch_layer(feats, weight, lists, n_out)}
    med, t, last = alternate(sides, blocks, reps)
    err = float((last["hip"] - last["torch"]).abs().max() / last["torch"].abs().max())
    flop = 2.0 * present * cin * cout
    nbytes = present * cin * 4.0 + n_out * cout * 4.0
    lines.append(f"{name}: {feats.shape[0]} -> {n_out} rows, {kvol} offsets, {present} present neighbours ({present / max(n_out, 1):.1f} per row), "
                 f"Cin {cin}, Cout {cout}")
    lines.append(f"  hip   {med['hip']:9.1f} us   {flop / med['hip'] * 1e-6:7.2f} TF = {100 * flop / med['hip'] * 1e-6 / PEAK_TF:5.1f} % of {PEAK_TF:g} TF   "
                 f"{nbytes / med['hip'] * 1e-6:6.3f} TB/s = {100 * nbytes / med['hip'] * 1e-6 / PEAK_TBS:5.1f} % of {PEAK_TBS:g} TB/s")
    lines.append(f"  torch {med['torch']:9.1f} us   ratio torch / hip = {med['torch'] / med['hip']:.2f}   max |hip - torch| / max |torch| = {err:.2e}")
    if med["hip"] >= med["torch"]:
        lines.append("  NOTE: the HIP layer is NOT faster than the torch composition here.")
    if map_fn is not None:
        m_us, _ = block_us(map_fn, reps)
        m_us = statistics.median([block_us(map_fn, reps)[0] for _ in range(blocks)])
        lines.append(f"  kernel map (one call, host wait for the row count included) {m_us:9.1f} us; map + convolution {m_us + med['hip']:9.1f} us")
    for k in sides:
        lines.append(f"  {k} blocks (us): {[round(x, 1) for x in t[k]]}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--pairs", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sparse_conv.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sparse_conv_time.py measures on a GPU: none found")
    from bench import build_module
    from proxytransformation_amd import sparse
    from proxytransformation_amd.pipeline import level_coordinates
    from proxytransformation_amd.synth import CONFIGS
    device = torch.device("cuda:0")
    mod, _ = build_module(CONFIGS["cfg4_room"], device)
    gen = torch.Generator(device=device).manual_seed(7)
    lines = [f"sparse convolution on the voxel rows, {B} room clouds x {N} points at {VOXEL * 100:g} cm; {torch.cuda.get_device_name(0)}; "
             f"median of {args.blocks} blocks of {args.reps} calls, sides alternating"]
    with torch.no_grad():
        outs = [torch.from_numpy(room_points(900 + b, N)).to(device) for b in range(B)]
        coords, feats3, ends = mod.quantize(outs, VOXEL, return_scene_rows=True)
        rnd = lambda *shape: torch.randn(shape, generator=gen, device=device)          # noqa: E731
        stem_map = lambda: sparse.kernel_map(coords, ends, 1, 3, 2)                      # noqa: E731
        layer_report("stem", feats3.contiguous(), stem_map(), rnd(27, 3, 64) / 9.0, args.blocks, args.reps, lines, map_fn=stem_map)
        c8, _, e8 = level_coordinates(coords, ends, 8, VOXEL)
        layer_report("64x64 at stride 8", rnd(c8.shape[0], 64), sparse.kernel_map(c8, e8, 8, 3, 1), rnd(27, 64, 64) / 41.6, args.blocks,
                     args.reps, lines)
        c64, _, e64 = level_coordinates(c8, e8, 64, VOXEL)
        layer_report("512x512 at stride 64", rnd(c64.shape[0], 512), sparse.kernel_map(c64, e64, 64, 3, 1), rnd(27, 512, 512) / 117.6,
                     args.blocks, args.reps, lines)
    if args.pairs and os.path.exists(args.pairs):
        lines.append("")
        lines.append("accuracy pairs of tests/test_gpu_sparse_conv.py: max |x - float64 restatement| / max |restatement| of the kernel (gpu) and of "
                     "the same fp32 chain on the CPU; the bar is gpu <= 8 x fp32-cpu")
        lines += [ln[ln.index("sparse_conv "):].rstrip() for ln in open(args.pairs) if ln.lstrip(". ").startswith("sparse_conv ")]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
