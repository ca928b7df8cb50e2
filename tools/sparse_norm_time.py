#!/usr/bin/env python3
"""Time the norm kernels on the voxel rows (proxytransformation_amd/sparse.py: ptx_sparse_norm_fwd / ptx_sparse_norm_bwd) and the eval
forward of the assembled MinkResNet-34, and write the report profiles/sparse_norm.txt keeps.

Shapes: 400 000 x 64 rows in 6 segments (the stem's instance norm at 1 cm voxels) and 20 000 x 256 rows in 6 segments.  Per shape
  instance norm   6 segments, weight + bias + ReLU          against  per-scene ``var_mean`` + elementwise + ``relu`` in torch;
  batch norm      1 segment, training, + residual + ReLU    against  ``nn.BatchNorm1d`` + add + ``relu`` in torch;
each forward alone (no autograd), forward + backward (autograd on both sides, gradients to the rows, weight, bias and the
residual), and the backward alone: the --reps forwards of a block are recorded before the block's first event, the block times the
``torch.autograd.grad`` calls only.  Every call READS its own set of buffers out of a ring larger than the 256 MiB Infinity Cache, so
the rows that are read come from HBM.  What a call WRITES -- the result, ``stats``, the workspace, the gradients -- is allocated by
the call, and the caching allocator hands back the addresses of a call or two before: the ring does not cover the written pass.
HIP events around blocks of --reps calls, the two sides alternating from block to block, block 0 a warm-up, reported = median of
the blocks.  A time is that of whole calls as a user makes them: the Python wrapper, ctypes, ``torch.empty`` of the outputs and
autograd's bookkeeping are inside it on both sides.  Beside each time: the bytes the kernels must move (row passes x n x C x 4) and
their share of the 6.3 TB/s a streaming kernel reaches on this chip.

Then one line for the eval forward of ``MinkResNet(34, 3)`` on six room clouds of 100 000 points quantised at 1 cm, split by events
that forward hooks on the first and the last block of every stage record.

Usage:  python tools/sparse_norm_time.py [--blocks 5] [--reps 8] [--out profiles/sparse_norm.txt]
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from sparse_conv_time import B, N, VOXEL, alternate, block_us, room_points      # noqa: E402

HBM_TBS = 6.3                       # what a float4 copy reaches on an MI355X
RING_BYTES = 640 << 20


def torch_instance_norm(x, ends, weight, bias):
    parts, lo = [], 0
    for hi in ends:
        if hi > lo:
            seg = x[lo:hi]
            var, mean = torch.var_mean(seg, dim=0, unbiased=False, keepdim=True)
            parts.append((seg - mean) * torch.rsqrt(var + 1e-8))
        lo = hi
    return torch.relu(torch.cat(parts) * weight + bias)


def ring(make, per_set_bytes):
    k = max(2, -(-RING_BYTES // per_set_bytes))
    sets = [make() for _ in range(k)]
    state = {"i": 0}

    def nxt():
        state["i"] = (state["i"] + 1) % k
        return sets[state["i"]]
    return nxt, k


def alternate_bwd(sides, blocks, reps):
    """``alternate`` for the backward alone.  {name: fn -> (outputs, inputs, grad_outputs)}: a block's forwards run before its first
    event, the block is ``reps`` calls of ``torch.autograd.grad`` on them."""
    names = list(sides)
    t = {k: [] for k in names}
    for blk in range(blocks + 1):
        for k in (names if blk % 2 == 0 else names[::-1]):
            graphs = iter([sides[k]() for _ in range(reps)])
            us, _ = block_us(lambda: torch.autograd.grad(*next(graphs)), reps)
            if blk:
                t[k].append(us)
    return {k: statistics.median(v) for k, v in t.items()}, t


def shape_report(n, C, S, blocks, reps, lines, gen):
    from proxytransformation_amd import sparse
    dev = torch.device("cuda:0")
    ends = [n * (s + 1) // S for s in range(S)]
    rows_bytes = n * C * 4
    rnd = lambda *shape: torch.randn(shape, generator=gen, device=dev)          # noqa: E731
    weight, bias = (torch.rand(C, generator=gen, device=dev) + 0.5), rnd(C)
    lines.append(f"{n} x {C} rows in {S} segments ({rows_bytes / 2 ** 20:.1f} MiB per pass over the rows)")

    def line(name, med, t, passes_hip):
        nbytes = passes_hip * rows_bytes
        lines.append(f"  {name:<34s} hip {med['hip']:8.1f} us   torch {med['torch']:8.1f} us   torch / hip = {med['torch'] / med['hip']:5.2f}   "
                     f"hip moves {passes_hip} row passes = {nbytes / 2 ** 20:.0f} MiB -> {nbytes / med['hip'] * 1e-6:5.2f} TB/s = "
                     f"{100 * nbytes / med['hip'] * 1e-6 / HBM_TBS:5.1f} % of {HBM_TBS} TB/s")
        for k in ("hip", "torch"):
            lines.append(f"    {k} blocks (us): {[round(v, 1) for v in t[k]]}")

    # ---- instance norm: forward alone, then forward + backward
    nxt, k = ring(lambda: rnd(n, C), 2 * rows_bytes)
    lines.append(f"  (ring of {k} buffer sets)")
    with torch.no_grad():
        med, t, last = alternate({"hip": lambda: sparse.sparse_segment_norm(nxt(), ends, 1e-8, weight, bias, relu=True),
                                  "torch": lambda: torch_instance_norm(nxt(), ends, weight, bias)}, blocks, reps)
    line("instance norm + ReLU, forward", med, t, 3)
    w_g, b_g = weight.clone().requires_grad_(), bias.clone().requires_grad_()
    nxt_g, _ = ring(lambda: (rnd(n, C).requires_grad_(), rnd(n, C)), 2 * rows_bytes)

    def hip_f():
        x, g = nxt_g()
        return sparse.sparse_segment_norm(x, ends, 1e-8, w_g, b_g, relu=True, differentiable=True), (x, w_g, b_g), g

    def torch_f():
        x, g = nxt_g()
        return torch_instance_norm(x, ends, w_g, b_g), (x, w_g, b_g), g

    med, t, _ = alternate({"hip": lambda: torch.autograd.grad(*hip_f()), "torch": lambda: torch.autograd.grad(*torch_f())}, blocks, reps)
    line("instance norm + ReLU, fwd + bwd", med, t, 3 + 7)
    med, t = alternate_bwd({"hip": hip_f, "torch": torch_f}, blocks, reps)
    line("instance norm + ReLU, backward", med, t, 7)       # g, x, out read twice, dx written

    # ---- training batch norm + residual + ReLU
    bn_h, bn_t = torch.nn.BatchNorm1d(C).to(dev).train(), torch.nn.BatchNorm1d(C).to(dev).train()
    nxt2, _ = ring(lambda: (rnd(n, C), rnd(n, C)), 3 * rows_bytes)
    with torch.no_grad():
        def hip_bn():
            x, r = nxt2()
            return sparse.sparse_batch_norm(x, bn_h, residual=r, relu=True)

        def torch_bn():
            x, r = nxt2()
            return torch.relu(bn_t(x) + r)
        med, t, _ = alternate({"hip": hip_bn, "torch": torch_bn}, blocks, reps)
    line("batch norm + residual + ReLU, fwd", med, t, 4)
    nxt3, _ = ring(lambda: (rnd(n, C).requires_grad_(), rnd(n, C).requires_grad_(), rnd(n, C)), 3 * rows_bytes)

    def hip_bn_f():
        x, r, g = nxt3()
        return sparse.sparse_batch_norm(x, bn_h, residual=r, relu=True, differentiable=True), (x, r, bn_h.weight, bn_h.bias), g

    def torch_bn_f():
        x, r, g = nxt3()
        return torch.relu(bn_t(x) + r), (x, r, bn_t.weight, bn_t.bias), g

    med, t, _ = alternate({"hip": lambda: torch.autograd.grad(*hip_bn_f()), "torch": lambda: torch.autograd.grad(*torch_bn_f())}, blocks, reps)
    line("batch norm + residual + ReLU, f + b", med, t, 4 + 7)
    med, t = alternate_bwd({"hip": hip_bn_f, "torch": torch_bn_f}, blocks, reps)
    line("batch norm + residual + ReLU, bwd", med, t, 7)    # g, x, out read, dresidual written; dresidual, x read, dx written


def backbone_report(blocks, lines):
    from bench import build_module
    from proxytransformation_amd import MinkResNet
    from proxytransformation_amd.synth import CONFIGS
    dev = torch.device("cuda:0")
    mod, _ = build_module(CONFIGS["cfg4_room"], dev)
    torch.manual_seed(0)
    net = MinkResNet(34, 3).to(dev).eval()
    with torch.no_grad():
        pts = [torch.from_numpy(room_points(900 + b, N)).to(dev) for b in range(B)]
        coords, feats3, ends = mod.quantize(pts, VOXEL, return_scene_rows=True)
        feats3 = feats3.contiguous()
        # an event before a stage's first block and one after its last: what lies before layer1's first block is the stem and
        # layer1's three kernel maps; a later stage's maps lie between the stage before and its own first block
        names = ["stem + maps 1", "layer1"] + [k for i in range(2, 5) for k in (f"maps {i}", f"layer{i}")]
        per = {k: [] for k in names}
        total = []
        rows = None
        ev = []

        def mark(*_):
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            ev.append(e)
        for i in range(4):
            stage = getattr(net, f"layer{i + 1}")
            stage[0].register_forward_pre_hook(mark)
            stage[len(stage) - 1].register_forward_hook(mark)
        for blk in range(blocks + 1):
            del ev[:]
            torch.cuda.synchronize()
            mark()
            outs = net(coords, ends, feats3)
            ev[-1].synchronize()
            rows = [int(lv.feats.shape[0]) for lv in outs]
            if blk:
                for k, a, b in zip(names, ev[:-1], ev[1:]):
                    per[k].append(a.elapsed_time(b))
                total.append(ev[0].elapsed_time(ev[-1]))
    lines.append(f"MinkResNet(34, 3) eval forward, {B} room clouds x {N} points at {VOXEL * 100:g} cm: {coords.shape[0]} rows -> levels of {rows} rows; "
                 f"median of {blocks} forwards {statistics.median(total):.2f} ms = " +
                 " + ".join(f"{k} {statistics.median(v):.2f}" for k, v in per.items()) + " ms (maps: the stage's kernel maps and their host waits)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sparse_norm.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sparse_norm_time.py measures on a GPU: none found")
    gen = torch.Generator(device="cuda:0").manual_seed(7)
    lines = [f"norm kernels on the voxel rows; {torch.cuda.get_device_name(0)}; median of {args.blocks} blocks of {args.reps} calls, sides "
             f"alternating, every call reads its own buffers out of a ring of at least {RING_BYTES >> 20} MiB and allocates what it writes; whole "
             f"calls through Python"]
    for n, C in ((400000, 64), (20000, 256)):
        shape_report(n, C, 6, args.blocks, args.reps, lines, gen)
    backbone_report(args.blocks, lines)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
