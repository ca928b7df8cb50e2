#!/usr/bin/env python3
"""Time the backward of batch_point_sample (ptx_point_sample_bwd) at the detector's shapes against torch autograd through an
F.grid_sample restatement, and write the report profiles/point_sample_bwd.txt keeps.

Workload: the four FPN_LEVELS of six cfg4_room scenes (V = 50 views), points = the level coordinates the chained pipeline
(GroundingFeaturePrefix) produces for those scenes.  Timed: the backward alone (torch.autograd.grad on a graph built before the
clock starts), HIP events on one stream.  Method: A/B interleaved per scene (the six scenes rotate the inputs), the order of the
two sides alternating from block to block, per-level time = sum over the scenes, reported = median of the blocks.

Also timed, per level: k_feat_transpose (prepare_features) on the same number of bytes, the yardstick for the gradient write;
and, with --rocprof, a `rocprofv3 --kernel-trace --stats` table of the HIP side alone per level (a fresh child process each).

Usage (on a GPU):  python tools/point_sample_bwd_time.py [--blocks 7] [--rocprof] [--out profiles/point_sample_bwd.txt]
"""
from __future__ import annotations

import argparse
import csv
import glob
import os
import subprocess
import sys
import tempfile

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PAD = (480, 480)            # GroundingFeaturePrefix's default img_pad_shape
HBM_PEAK_GBS = 8000.0       # MI355X: HBM3E 8.0 TB/s spec (bench.py uses the same figure)


def make_inputs(B, device):
    """Level points [level][scene] (n,3) and projection matrices [scene] (V,4,4) from one chained pipeline call."""
    from bench import build_module
    from proxytransformation_amd.pipeline import GroundingFeaturePrefix, projection_matrices
    from proxytransformation_amd.synth import CONFIGS, FPN_LEVELS, make_depth_scene
    cfg = CONFIGS["cfg4_room"]
    mod, _ = build_module(cfg, device)
    scenes_np = [make_depth_scene(cfg.seed_base + 50 + b, V=cfg.V) for b in range(B)]
    scenes = [dict(sc, depth_img=torch.from_numpy(sc["depth_img"].view(np.int16)).to(device).view(torch.uint16)) for sc in scenes_np]
    g = torch.Generator(device=device)
    g.manual_seed(cfg.seed_base)
    feats = [torch.randn((B, cfg.V, c, s, s), generator=g, device=device) for c, s in FPN_LEVELS]
    text = {"text_feats": torch.randn((B, cfg.L, cfg.embed_dim), generator=g, device=device),
            "text_token_mask": torch.ones((B, cfg.L), dtype=torch.bool, device=device)}
    res = GroundingFeaturePrefix(mod, n_points=cfg.N)(scenes, text, feats, rng=np.random.RandomState(0))
    torch.cuda.synchronize()
    points = [[p.clone() for p in lvl] for lvl in res.level_points]
    proj = [torch.from_numpy(projection_matrices(sc["depth2img"])).to(device) for sc in scenes_np]
    return points, proj


def restatement(feats, pts, proj):
    """batch_point_sample as differentiable torch (point_fusion.py:208-313 as the detector calls it: nearest, zeros padding,
    align_corners, valid_flag; no image augmentation): the baseline whose backward torch's autograd provides."""
    V = feats.shape[0]
    q = torch.einsum("vrk,nk->vnr", proj, torch.cat([pts, pts.new_ones(len(pts), 1)], 1))
    z = q[..., 2].clamp(min=1e-3)
    cx, cy = q[..., 0] / z, q[..., 1] / z
    grid = torch.stack([cx / PAD[1] * 2 - 1, cy / PAD[0] * 2 - 1], -1).view(V, 1, -1, 2)
    samp = F.grid_sample(feats, grid, mode="nearest", padding_mode="zeros", align_corners=True)
    valid = ((cx < PAD[1]) & (cx > 0) & (cy < PAD[0]) & (cy > 0) & (q[..., 2] > 0)).sum(0)
    return (samp.squeeze(2).sum(0).t() / valid.clamp(min=1)[:, None]) * (valid > 0)[:, None]


def ours(feats, pts, proj):
    from proxytransformation_amd.fusion import batch_point_sample
    return batch_point_sample(None, feats, pts, proj, "DEPTH", img_pad_shape=PAD, img_shape=PAD, aligned=False)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    r = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), r


def run_level(li, points, proj, blocks, hip_only, device):
    """-> dict of per-level medians (ms, summed over the scenes)."""
    from proxytransformation_amd.fusion import prepare_features
    from proxytransformation_amd.synth import CONFIGS, FPN_LEVELS
    C, S = FPN_LEVELS[li]
    V, B = CONFIGS["cfg4_room"].V, len(proj)
    g = torch.Generator(device=device)
    g.manual_seed(100 + li)
    t_hip, t_ref, t_tr = [], [], []
    worst = 0.0
    for blk in range(blocks + 1):                      # block 0 warms up
        s_hip = s_ref = s_tr = 0.0
        for b in range(B):
            pts = points[li][b]
            f = torch.randn((V, C, S, S), generator=g, device=device).requires_grad_()
            dout = torch.randn((len(pts), C), generator=g, device=device)
            sides = ["hip"] if hip_only else (["hip", "ref"] if blk % 2 == 0 else ["ref", "hip"])
            grads = {}
            for side in sides:
                out = (ours if side == "hip" else restatement)(f, pts, proj[b])
                torch.cuda.synchronize()
                ms, (gr,) = timed(lambda: torch.autograd.grad(out, f, dout))
                grads[side] = gr
                if side == "hip":
                    s_hip += ms
                else:
                    s_ref += ms
                del out
            if len(grads) == 2 and blk == 0:
                # the restatement's fp32 projection is not the pinned order of the kernels: a point on a pixel-rounding boundary lands
                # on the neighbouring pixel there, so a few elements differ by a whole term; everything else agrees to rounding
                off = (grads["hip"] - grads["ref"]).abs() > 1e-5 * grads["ref"].abs().max()
                worst = max(worst, float(off.float().mean()))
            grads.clear()
            ms, ws = timed(lambda: prepare_features(f.detach()))
            s_tr += ms
            del ws, f, dout
        if blk:
            t_hip.append(s_hip); t_ref.append(s_ref); t_tr.append(s_tr)
    med = lambda v: float(np.median(v)) if v else float("nan")
    return dict(level=li, C=C, S=S, rows=[len(p) for p in points[li]], grad_bytes=B * V * C * S * S * 4, hip_ms=med(t_hip),
                ref_ms=med(t_ref), transpose_ms=med(t_tr), hip_blocks=t_hip, ref_blocks=t_ref, differ=worst)


def rocprof_table(inputs_path, li):
    """One child under rocprofv3 (--kernel-trace --stats), HIP side only, one level: rows of the backward's kernels."""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "k", "--", sys.executable,
               os.path.abspath(__file__), "--child", inputs_path, "--level", str(li), "--blocks", "3"]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if r.returncode != 0 or not files:
            return [f"  (rocprofv3 run failed: exit {r.returncode}: {r.stderr.strip().splitlines()[-1:] or ''})"]
        rows = [x for x in csv.DictReader(open(files[0])) if "psb" in x["Name"] or "point_sample" in x["Name"] or "feat_transpose" in x["Name"]]
    lines = [f"  {'kernel':<44}{'calls':>7}{'avg us':>10}{'min us':>10}{'max us':>10}"]
    for x in rows:
        name = x["Name"].split("(")[0].replace("void ptx::", "")
        lines.append(f"  {name:<44}{x['Calls']:>7}{float(x['AverageNs']) / 1e3:>10.1f}{float(x['MinNs']) / 1e3:>10.1f}"
                     f"{float(x['MaxNs']) / 1e3:>10.1f}")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--scenes", type=int, default=6)
    ap.add_argument("--rocprof", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, help="(internal) inputs file: HIP side only, for the rocprofv3 child")
    ap.add_argument("--level", type=int, default=None)
    args = ap.parse_args()
    device = torch.device("cuda:0")
    if args.child:
        d = torch.load(args.child, map_location=device)
        run_level(args.level, d["points"], d["proj"], args.blocks, True, device)
        return
    points, proj = make_inputs(args.scenes, device)
    levels = range(4) if args.level is None else [args.level]
    res = [run_level(li, points, proj, args.blocks, False, device) for li in levels]
    out = []
    out.append(f"point-sample backward, {args.scenes} cfg4_room scenes x 50 views, nearest; {torch.cuda.get_device_name(0)}; "
               f"median of {args.blocks} blocks, A/B interleaved per scene, ms summed over the scenes")
    out.append(f"{'level':>5}{'C':>5}{'HxW':>9}{'rows/scene':>12}{'grad MB':>9}{'HIP ms':>9}{'torch ms':>10}{'torch/HIP':>10}"
               f"{'HIP GB/s':>10}{'of peak':>8}{'transp ms':>10}{'transp GB/s wr':>15}{'differ':>10}")
    for r in res:
        gbs = r["grad_bytes"] / r["hip_ms"] / 1e6
        tgbs = r["grad_bytes"] / r["transpose_ms"] / 1e6
        out.append(f"{r['level']:>5}{r['C']:>5}{r['S']:>5}x{r['S']:<3}{int(np.mean(r['rows'])):>12}{r['grad_bytes'] / 1e6:>9.0f}"
                   f"{r['hip_ms']:>9.3f}{r['ref_ms']:>10.3f}{r['ref_ms'] / r['hip_ms']:>10.2f}{gbs:>10.0f}{gbs / HBM_PEAK_GBS:>8.1%}"
                   f"{r['transpose_ms']:>10.3f}{tgbs:>15.0f}{r['differ']:>10.1e}")
    out.append("HIP ms: the whole backward (index build + gradient write); GB/s = gradient bytes written / that time; of peak: of "
               f"{HBM_PEAK_GBS / 1e3:.1f} TB/s.  transp: k_feat_transpose (prepare_features) on the same bytes (it reads as many).  differ: share of "
               "gradient elements off by more than 1e-5 of the largest against torch (points ON a pixel-rounding boundary: torch's "
               "projection is not the pinned fp32 order).")
    for r in res:
        out.append(f"level {r['level']} blocks (ms): HIP {[round(x, 3) for x in r['hip_blocks']]}  torch {[round(x, 3) for x in r['ref_blocks']]}")
    if args.rocprof:
        with tempfile.TemporaryDirectory() as d:
            path = os.path.join(d, "inputs.pt")
            torch.save(dict(points=points, proj=proj), path)
            for li in levels:
                out.append(f"rocprofv3 --kernel-trace --stats, level {li}, HIP side only (one call per scene, 4 blocks):")
                out += rocprof_table(path, li)
    text = "\n".join(out) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
