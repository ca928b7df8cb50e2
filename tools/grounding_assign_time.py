#!/usr/bin/env python3
"""Time the two matchers of the grounding loss (proxytransformation_amd/grounding_loss.py: ``GroundingLoss(matcher=...).assign``) on an
MI355X and write the report profiles/grounding_assign.txt keeps.

Both matchers run in one process on the same inputs, whole calls through Python:

* ``matcher='device'`` (``ptx_gl_cost`` + ``ptx_gl_assign``, no host wait): the STREAM time of a call by HIP events around a block of
  calls, and the HOST time of a call (``perf_counter`` around the same block before anything is waited for: what enqueueing costs);
* ``matcher='host'`` (``ptx_gl_cost``, one copy, one synchronise, scipy per (layer, scene), one copy back): the WALL time of a call,
  its synchronise included -- the host cannot enqueue anything behind it earlier;
* the cost launch alone (``match_costs``) by events: what both matchers share.

Shapes: the shipped one (6 layers, 6 scenes, 256 queries, 77 text tokens of 256) with 1 to 4, 16 and 64 ground-truth boxes per scene,
and one at the device solver's limit (1024 queries, 256 boxes; 2 layers, 2 scenes).  N(0, 2) scores with ``-inf`` on the masked columns,
random boxes.  Per figure: the median of --blocks blocks of --reps calls after a warm-up block, the matchers alternating, with the range
of the blocks.

Usage (on a GPU):  python tools/grounding_assign_time.py [--blocks 7] [--reps 10] [--out profiles/grounding_assign.txt]
"""
from __future__ import annotations

import argparse
import math
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

T, M = 77, 256
SHAPES = (("shipped, 1-4 boxes", 6, 6, 256, (1, 4, 2, 3, 1, 2)), ("shipped, 16 boxes", 6, 6, 256, (16,) * 6),
          ("shipped, 64 boxes", 6, 6, 256, (64,) * 6), ("limit, 1024 x 256", 2, 2, 1024, (256, 256)))


def inputs(NL, B, K, G, dev, seed=0):
    rng = np.random.default_rng(seed)
    mask = np.zeros((B, T), bool)
    for b in range(B):
        mask[b, :int(rng.integers(10, T + 1))] = True
    scores = np.full((NL, B, K, M), -np.inf, np.float32)
    scores[..., :T] = np.where(mask[None, :, None, :], rng.normal(0.0, 2.0, (NL, B, K, T)), -np.inf)
    box = lambda *s: np.concatenate([rng.normal(0.0, 1.0, s + (3,)), rng.uniform(0.2, 1.5, s + (3,)), rng.uniform(-math.pi, math.pi, s + (3,))], -1)      # noqa: E731
    boxes = box(NL, B, K).astype(np.float32)
    gts = [box(g).astype(np.float32) for g in G]
    pms = []
    for b in range(B):
        pm = np.zeros((G[b], M), np.float32)
        for i in range(G[b]):
            pm[i, rng.permutation(int(mask[b].sum()))[:2]] = 0.5
        pms.append(pm)
    put = lambda a: torch.from_numpy(a).to(dev)      # noqa: E731
    return put(scores), put(boxes), put(mask), [put(g) for g in gts], [put(p) for p in pms]


def block(fn, reps):
    """``(stream us per call, host us per call up to the last enqueue, wall us per call, last result)`` of ``reps`` calls."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a.record()
    for _ in range(reps):
        r = fn()
    b.record()
    t1 = time.perf_counter()
    b.synchronize()
    t2 = time.perf_counter()
    return 1e3 * a.elapsed_time(b) / reps, 1e6 * (t1 - t0) / reps, 1e6 * (t2 - t0) / reps, r


def alternate(sides, blocks, reps):
    """``{name: fn} -> ({name: [(stream, host, wall) per block]}, {name: last result})``; block 0 warms up, the order flips per block."""
    names = list(sides)
    t, last = {k: [] for k in names}, {}
    for blk in range(blocks + 1):
        for k in (names if blk % 2 == 0 else names[::-1]):
            *us, last[k] = block(sides[k], reps)
            if blk:
                t[k].append(us)
    return t, last


def figure(values):
    return f"{statistics.median(values):9.1f} us (min {min(values):.1f}, max {max(values):.1f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grounding_assign.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("grounding_assign_time.py measures on a GPU: none found")
    from proxytransformation_amd import GroundingLoss, grounding_loss as gl
    dev = torch.device("cuda:0")
    host, device = GroundingLoss(matcher="host"), GroundingLoss(matcher="device")
    lines = [f"matching of the grounding loss, matcher='device' (ptx_gl_cost + ptx_gl_assign) against matcher='host' (ptx_gl_cost, copy, "
             f"synchronise, scipy); {torch.cuda.get_device_name(0)}; {T} text tokens of {M}",
             f"whole calls through Python (GroundingLoss.assign), median of {args.blocks} blocks of {args.reps} calls after a warm-up block, "
             "matchers alternating",
             "stream: HIP events around the block; host: perf_counter up to the last enqueue; wall: up to the end of the block's last call"]
    for name, NL, B, K, G in SHAPES:
        ops = inputs(NL, B, K, G, dev)
        with torch.no_grad():
            t, last = alternate({"device": lambda: device.assign(*ops), "host": lambda: host.assign(*ops),
                                 "cost": lambda: gl.match_costs(*ops)[0]}, args.blocks, args.reps)
        col = lambda k, i: [row[i] for row in t[k]]      # noqa: E731
        stream, wall = statistics.median(col("device", 0)), statistics.median(col("host", 2))
        same = int((last["device"] == last["host"]).sum())
        lines.append(f"{name}: {NL} layers, {B} scenes, {K} queries, {list(G)} boxes per scene")
        lines.append(f"  device  stream {figure(col('device', 0))}   host (enqueue only) {figure(col('device', 1))}")
        lines.append(f"  host    wall   {figure(col('host', 2))}   (its synchronise included)")
        lines.append(f"  cost launch alone, stream {figure(col('cost', 0))}")
        lines.append(f"  host wall / device stream {wall / stream:6.2f}" + ("   the device matcher is BEHIND the host path here" if stream > wall else "")
                     + f"; assignments equal at {same} of {last['host'].numel()} places")
    text_out = "\n".join(lines) + "\n"
    print(text_out, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text_out)


if __name__ == "__main__":
    main()
