#!/usr/bin/env python3
"""Time the differentiable voxel quantisation (module.quantize with grad mode on: ptx_voxelize_rep + ptx_voxel_features_bwd) and
write the report profiles/voxel_features_bwd.txt keeps.

Part 1, the operator: six clouds of 100 000 points (the surfaces of a 7 x 5 x 3 m room, 1 cm voxels: a few per cent of the points
share a voxel), one padded (6,N,3) buffer as the neck hands it over.  Timed, forward and backward apart, HIP events on one stream:
  hip     quantize(outs) with grad -> features; torch.autograd.grad(features, outs, dfeats)
  torch   what a user writes without it: the plain quantize(return_inverse=True), the first index per row from the inverse map
          (scatter_reduce amin), features = torch.cat(outs)[rep]; the same torch.autograd.grad
  gather  the torch form's differentiable part alone (rep precomputed): torch.cat(outs)[rep] and its backward
The gradients of the three are compared bit for bit.  Method: one warm-up block, then blocks of --reps calls per side, the order
of the sides rotating from block to block, reported = median of the blocks.

Part 2, the training step at the reference's training shape (bench.py's train_step_ms configuration: 6 scenes, 100k points, gs 12,
3 + 3 blocks, 20 views): the step with the upstream gradients arriving on ``outs`` directly -- all the parent could do -- beside
the step with them arriving on the voxel features behind quantize.  Host clock around blocks of steps that end in a synchronise,
A/B alternating, median of the blocks.

Usage (on a GPU):  python tools/voxel_grad_time.py [--blocks 7] [--reps 20] [--steps 20] [--out profiles/voxel_features_bwd.txt]
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
B, N, VOXEL = 6, 100000, 0.01


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


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    r = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), r


def operator_part(mod, device, blocks, reps, lines):
    base = torch.from_numpy(np.stack([room_points(900 + b, N) for b in range(B)])).to(device).requires_grad_(True)
    outs = [base[b, :N - 37 * b] for b in range(B)]              # ragged like the neck's outputs; views of one padded buffer
    total = sum(int(o.shape[0]) for o in outs)
    with torch.no_grad():
        coords, _ = mod.quantize(outs, VOXEL)
    nvox = int(coords.shape[0])
    dfeats = torch.randn((nvox, 3), generator=torch.Generator(device=device).manual_seed(3), device=device)
    ar = torch.arange(total, device=device)

    def rep_of(inv):
        return torch.full((nvox,), total, dtype=torch.int64, device=device).scatter_reduce_(0, torch.cat(inv).long(), ar, "amin")

    with torch.no_grad():
        rep0 = rep_of(mod.quantize(outs, VOXEL, return_inverse=True)[2])

    def fwd_hip():
        return mod.quantize(outs, VOXEL)[1]

    def fwd_torch():
        with torch.no_grad():
            inv = mod.quantize(outs, VOXEL, return_inverse=True)[2]
            rep = rep_of(inv)
        return torch.cat(outs)[rep]

    def fwd_gather():
        return torch.cat(outs)[rep0]

    sides = {"hip": fwd_hip, "torch": fwd_torch, "gather": fwd_gather}
    names = list(sides)
    t = {k: {"fwd": [], "bwd": []} for k in sides}
    grads = {}
    for blk in range(blocks + 1):                                  # block 0 warms up
        order = names[blk % 3:] + names[:blk % 3]
        for k in order:
            f_ms = b_ms = 0.0
            for _ in range(reps):
                torch.cuda.synchronize()
                ms, f = timed(sides[k])
                f_ms += ms
                ms, g = timed(lambda: torch.autograd.grad(f, outs, dfeats))
                b_ms += ms
                grads[k] = g
            if blk:
                t[k]["fwd"].append(1e3 * f_ms / reps)
                t[k]["bwd"].append(1e3 * b_ms / reps)
    same = all(torch.equal(a, b) and torch.equal(a, c) for a, b, c in zip(grads["hip"], grads["torch"], grads["gather"]))
    med = {k: {p: statistics.median(v[p]) for p in v} for k, v in t.items()}
    lines.append(f"differentiable quantize, {B} clouds x {N} points ({total} rows in, {nvox} voxels at {VOXEL * 100:g} cm, "
                 f"{total - nvox} duplicates); {torch.cuda.get_device_name(0)}; median of {blocks} blocks of {reps} calls, sides rotating")
    lines.append(f"{'side':8s} {'fwd us':>9s} {'bwd us':>9s} {'fwd+bwd us':>11s}   vs hip (fwd+bwd)   vs hip (bwd)")
    hip = med["hip"]
    for k in names:
        m = med[k]
        lines.append(f"{k:8s} {m['fwd']:9.1f} {m['bwd']:9.1f} {m['fwd'] + m['bwd']:11.1f}   {(m['fwd'] + m['bwd']) / (hip['fwd'] + hip['bwd']):16.2f}   "
                     f"{m['bwd'] / hip['bwd']:12.2f}")
    lines.append("hip: quantize with grad + autograd.grad to the six outputs.  torch: plain quantize(return_inverse) + first index per row "
                 "(scatter_reduce amin) + torch.cat(outs)[rep] + autograd.grad.  gather: torch.cat(outs)[rep] alone, rep precomputed.")
    lines.append("HIP events around each call, so the times include the host's share of it.  the backward kernel moves "
                 f"{(total * (4 + 12) + nvox * (4 + 12)) / 1e6:.1f} MB.  gradients of the three sides bit-identical: {same}")
    if hip["fwd"] + hip["bwd"] >= med["torch"]["fwd"] + med["torch"]["bwd"]:
        lines.append("NOTE: the HIP path is NOT faster than the torch form here.")
    if hip["bwd"] >= med["gather"]["bwd"]:
        lines.append("NOTE: the HIP backward alone is NOT faster than the backward of torch.cat(outs)[rep].")
    for k in names:
        lines.append(f"{k} blocks (us): fwd {[round(x, 1) for x in t[k]['fwd']]}  bwd {[round(x, 1) for x in t[k]['bwd']]}")
    return same


def step_part(device, blocks, steps, lines):
    from proxytransformation_amd import MODELS
    from proxytransformation_amd.synth import PreshapeConfig, fill_state_dict, make_scene_batch
    cfg = PreshapeConfig("cfg4train", B=6, N=100000, grid_size=12, dynamic_drop_radio=0.6, L=20, V=20, text_blocks=3,
                         img_blocks=3, seed_base=4500)
    mod = MODELS.build(dict(type="ProxyTransformationNormReverse", **cfg.module_kwargs()))
    mod.load_state_dict({k: torch.from_numpy(v) for k, v in fill_state_dict(mod.state_dict()).items()})
    mod = mod.to(device).train()
    pts, text, mask, img = make_scene_batch(cfg)
    args = ([torch.from_numpy(p).to(device) for p in pts],
            {"text_feats": torch.from_numpy(text).to(device).requires_grad_(True), "text_token_mask": torch.from_numpy(mask).to(device)},
            torch.from_numpy(img).to(device).requires_grad_(True))
    leaves = list(mod.parameters()) + [args[1]["text_feats"], args[2]]
    gos = {}

    def step(behind):
        for t_ in leaves:
            t_.grad = None
        outs = mod(*args)
        if behind:                      # the upstream gradient arrives on the voxel features (the sparse backbone's input)
            feats = mod.quantize(outs, VOXEL)[1]
            key = ("f", feats.shape[0])
            if key not in gos:
                gos[key] = torch.ones_like(feats)
            feats.backward(gos[key])
        else:                           # ... on the neck's outputs: the step of bench.py's train_step_ms
            key = tuple(o.shape[0] for o in outs)
            if key not in gos:
                gos[key] = [torch.ones_like(o) for o in outs]
            torch.autograd.backward(outs, gos[key])

    for behind in (False, True):
        for _ in range(10):
            step(behind)
    vals = {False: [], True: []}
    for blk in range(blocks):
        for behind in ((False, True) if blk % 2 == 0 else (True, False)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                step(behind)
            torch.cuda.synchronize()
            vals[behind].append(1e3 * (time.perf_counter() - t0) / steps)
    a, b = statistics.median(vals[False]), statistics.median(vals[True])
    lines.append("")
    lines.append(f"training step, 6 scenes x 100k points, gs 12, 3 + 3 blocks, 20 views (fp32 features); host clock, blocks of {steps} steps, "
                 f"A/B alternating, median of {blocks} blocks")
    lines.append(f"  gradients arrive on outs (the parent's step)          {a:7.3f} ms")
    lines.append(f"  gradients arrive on the voxel features behind quantize {b:7.3f} ms   ({b - a:+.3f} ms)")
    lines.append(f"  blocks (ms): outs {[round(x, 3) for x in vals[False]]}  behind quantize {[round(x, 3) for x in vals[True]]}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "voxel_features_bwd.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("voxel_grad_time.py measures on a GPU: none found")
    from bench import build_module
    from proxytransformation_amd.synth import CONFIGS
    device = torch.device("cuda:0")
    mod, _ = build_module(CONFIGS["cfg4_room"], device)
    lines = []
    same = operator_part(mod, device, args.blocks, args.reps, lines)
    step_part(device, args.blocks, args.steps, lines)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    if not same:
        raise SystemExit("the gradients of the three sides differ")


if __name__ == "__main__":
    main()
