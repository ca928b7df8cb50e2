#!/usr/bin/env python3
"""Time the level join (fusion.join_level_features, one launch per level) against the route it replaces (one batch_point_sample
launch per scene, a torch.cat over the scenes and one over the channels), alone per level and inside GroundingDetector, and write
the report profiles/detector.txt keeps.

Shape (the README's): six scenes in a (7, 5, 3) m room, 50 views, the four FPN_LEVELS of image features, 100 000 points, 77 text
tokens, 256 queries, MinkResNet-34, 6 decoder layers.

Part A, the join alone: per level a synthetic sparse level of the row counts the chained pipeline reaches at that shape (distinct
voxels of the level's stride inside the room), the cameras of synth.make_depth_scene; forward, and forward + backward (gradients to
the level's features and to the image features), both routes on the SAME prepared channels-last copies (they are not part of
either side).  Part B, the detector: eval forward (predict) and training step (loss + backward) with fused_join on and off.
Method: HIP events on one stream, A/B interleaved, the order of the two sides alternating from block to block, block 0 warms up,
reported = median of the blocks.

Usage (on a GPU):  python tools/detector_time.py [--blocks 7] [--skip-detector] [--out profiles/detector.txt]
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PAD = (480, 480)
ROWS = (41228, 13125, 2679, 280)        # rows per scene and level: the pipeline's clouds at this shape (profiles/point_sample_bwd.txt);
                                        # level 3: every voxel of stride 64 inside the room
STRIDES = (8, 16, 32, 64)
VOXEL = 0.01
EXTENT = (7.0, 5.0, 3.0)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    r = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), r


def ab(sides: dict, blocks: int):
    """{name: fn} -> {name: [ms per block]}: interleaved, alternating order, block 0 dropped."""
    names = list(sides)
    out = {n: [] for n in names}
    for blk in range(blocks + 1):
        for n in (names if blk % 2 == 0 else names[::-1]):
            torch.cuda.synchronize()
            ms, _ = timed(sides[n])
            if blk:
                out[n].append(ms)
    return out


def scene_tables(B, V, device):
    from proxytransformation_amd.fusion import JoinTables
    from proxytransformation_amd.pipeline import projection_matrices
    from proxytransformation_amd.synth import make_depth_scene
    scenes = [make_depth_scene(4050 + b, V=V) for b in range(B)]
    projs = [projection_matrices(sc["depth2img"]) for sc in scenes]
    scal = [(0.75, 1.0, 0.0, 0.0, False, float(PAD[1]), float(PAD[0]), float(PAD[1]))] * B     # CFG:114: 480 x 640 resized to 480 x 480
    return scenes, JoinTables(projs, [None] * B, scal, VOXEL, device)


def synthetic_level(li, B, C, device, rng):
    from proxytransformation_amd.backbone import SparseLevel
    s = STRIDES[li]
    cells = [int(e / VOXEL) // s for e in EXTENT]
    total = cells[0] * cells[1] * cells[2]
    coords, ends = [], []
    for b in range(B):
        n = ROWS[li]
        assert n <= total, (li, n, total)
        flat = np.sort(rng.choice(total, n, replace=False))
        xyz = np.stack(np.unravel_index(flat, cells), 1) * s
        coords.append(np.concatenate([np.full((n, 1), b), xyz], 1).astype(np.int32))
        ends.append((ends[-1] if ends else 0) + n)
    coords = torch.from_numpy(np.concatenate(coords)).to(device)
    feats = torch.randn((ends[-1], C), device=device)
    return SparseLevel(feats=feats, coords=coords, scene_rows=ends, tensor_stride=s)


def join_alone(B, V, blocks, device):
    from proxytransformation_amd.fusion import join_level_features, join_level_features_per_scene, prepare_features_many
    from proxytransformation_amd.synth import FPN_LEVELS
    rng = np.random.default_rng(0)
    _, tables = scene_tables(B, V, device)
    rows = []
    for li, (C, S) in enumerate(FPN_LEVELS):
        level = synthetic_level(li, B, C, device, rng)
        img = torch.randn((B, V, C, S, S), device=device)
        prepared = prepare_features_many([img[b] for b in range(B)])
        g = torch.randn((level.feats.shape[0], 2 * C), device=device)
        fused = lambda lv=level, im=img: join_level_features(lv, im, tables, prepared=prepared)                      # noqa: E731
        per_scene = lambda lv=level, im=img: join_level_features_per_scene(lv, im, tables, prepared=prepared)             # noqa: E731
        with torch.no_grad():
            assert torch.equal(fused(), per_scene()), f"level {li}: the two routes differ"
            fwd = ab(dict(fused=fused, per_scene=per_scene), blocks)

        def step(route):
            f = level.feats.detach().requires_grad_()
            im = img.detach().requires_grad_()
            lv = type(level)(feats=f, coords=level.coords, scene_rows=level.scene_rows, tensor_stride=level.tensor_stride)
            (fused if route == "fused" else per_scene)(lv, im).backward(g)
            return f.grad, im.grad

        ga, gb = step("fused"), step("per_scene")
        assert torch.equal(ga[0], gb[0]) and torch.equal(ga[1], gb[1]), f"level {li}: the two backward routes differ"
        both = ab(dict(fused=lambda: step("fused"), per_scene=lambda: step("per_scene")), blocks)
        rows.append(dict(level=li, C=C, S=S, rows=level.scene_rows[0], fwd=fwd, both=both))
    return rows


def shipped_cfg():
    """configs/grounding/proxy-tiblock33-gs12-wbias-ddr0.6-clip.py, model= (CFG:19-100); CLIP ViT-L/14's text width is 768."""
    attn = dict(embed_dims=256, num_heads=8, dropout=0.0)
    return dict(
        preshape=dict(type="ProxyTransformationNormReverse", n_points=100000, grid_size=12, text_blocks=3, img_blocks=3,
                      dynamic_drop_radio=0.6, num_sub=30),
        backbone_3d=dict(type="MinkResNet", in_channels=3, depth=34), use_xyz_feat=True,
        neck_3d=dict(type="MinkNeck", num_classes=1, in_channels=[128, 256, 512, 1024], out_channels=256, voxel_size=VOXEL,
                     pts_prune_threshold=1000),
        decoder=dict(num_layers=6, return_intermediate=True, post_norm_cfg=None,
                     layer_cfg=dict(self_attn_cfg=dict(attn), cross_attn_text_cfg=dict(attn), cross_attn_cfg=dict(attn),
                                    ffn_cfg=dict(embed_dims=256, feedforward_channels=2048, ffn_drop=0.0))),
        bbox_head=dict(type="GroundingHead", num_classes=256, sync_cls_avg_factor=True, decouple_bbox_loss=True, decouple_groups=4,
                       share_pred_layer=True, decouple_weights=[0.2, 0.2, 0.2, 0.4],
                       contrastive_cfg=dict(max_text_len=256, log_scale="auto", bias=True)),
        num_queries=256, voxel_size=VOXEL, coord_type="DEPTH", text_width=768)


def detector_times(B, V, T, blocks, device):
    from proxytransformation_amd import GroundingDetector
    from proxytransformation_amd.synth import FPN_LEVELS
    torch.manual_seed(0)
    det = GroundingDetector(**shipped_cfg(), differentiable=True, matcher="device")
    with torch.no_grad():
        for p in det.parameters():
            if p.dim() >= 2:
                p.add_(torch.randn_like(p) * 0.02)
    det = det.to(device)
    scenes, _ = scene_tables(B, V, device)
    scenes = [dict(depth2img=sc["depth2img"], img_meta=sc.get("img_meta")) for sc in scenes]
    rng = np.random.default_rng(1)
    points = [torch.from_numpy(rng.random((100000, 3), dtype=np.float32) * np.asarray(EXTENT, np.float32)).to(device) for _ in range(B)]
    img = [torch.randn((B, V, c, s, s), device=device) for c, s in FPN_LEVELS]
    text = torch.randn((B, T, 768), device=device)
    mask = torch.ones((B, T), dtype=torch.bool, device=device)
    gt = [torch.tensor([[3.0, 2.0, 1.0, 0.8, 0.6, 0.5, 0.3, 0.0, 0.0], [1.5, 3.5, 0.8, 0.5, 0.9, 0.7, -0.5, 0.0, 0.0]], device=device)] * B
    pos = torch.zeros((2, 256), device=device)
    pos[0, 1:3] = 1.0
    pos[1, 4:6] = 1.0

    def predict(fused):
        det.eval()
        det.fused_join = fused
        return det.predict(points, text, mask, img, scenes, img_pad_shape=PAD)

    def train(fused):
        det.train()
        det.fused_join = fused
        det.zero_grad(set_to_none=True)
        losses = det.loss(points, text, mask, img, scenes, gt, [pos] * B, img_pad_shape=PAD)
        sum(losses.values()).backward()

    ev = ab(dict(fused=lambda: predict(True), per_scene=lambda: predict(False)), blocks)
    tr = ab(dict(fused=lambda: train(True), per_scene=lambda: train(False)), blocks)
    return ev, tr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--scenes", type=int, default=6)
    ap.add_argument("--views", type=int, default=50)
    ap.add_argument("--tokens", type=int, default=77)
    ap.add_argument("--skip-detector", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    device = torch.device("cuda:0")
    med = lambda v: float(np.median(v))          # noqa: E731
    out = [f"level join, {args.scenes} scenes x {args.views} views, nearest, fp32 features; {torch.cuda.get_device_name(0)}; median of "
           f"{args.blocks} blocks, A/B interleaved, order alternating; ms per level, all scenes",
           f"{'level':>5}{'Cb=Ci':>7}{'HxW':>9}{'rows/scene':>12}{'fwd fused':>11}{'fwd per-scene':>15}{'per/fused':>11}"
           f"{'fwd+bwd fused':>15}{'fwd+bwd per-scene':>19}{'per/fused':>11}"]
    rows = join_alone(args.scenes, args.views, args.blocks, device)
    for r in rows:
        f0, f1, b0, b1 = med(r["fwd"]["fused"]), med(r["fwd"]["per_scene"]), med(r["both"]["fused"]), med(r["both"]["per_scene"])
        out.append(f"{r['level']:>5}{r['C']:>7}{r['S']:>5}x{r['S']:<3}{r['rows']:>12}{f0:>11.3f}{f1:>15.3f}{f1 / f0:>11.2f}{b0:>15.3f}{b1:>19.3f}"
                   f"{b1 / b0:>11.2f}")
    tot = [sum(med(r[k][s]) for r in rows) for k, s in (("fwd", "fused"), ("fwd", "per_scene"), ("both", "fused"), ("both", "per_scene"))]
    out.append(f"all four levels: forward {tot[0]:.3f} ms fused, {tot[1]:.3f} ms per scene; forward + backward {tot[2]:.3f} ms fused, "
               f"{tot[3]:.3f} ms per scene.  Both routes read the same prepared channels-last copies (not timed) and give equal bits "
               "(asserted here, forward and backward).")
    for r in rows:
        out.append(f"level {r['level']} forward blocks (ms): fused {[round(x, 3) for x in r['fwd']['fused']]}  per-scene "
                   f"{[round(x, 3) for x in r['fwd']['per_scene']]}")
    if not args.skip_detector:
        ev, tr = detector_times(args.scenes, args.views, args.tokens, max(3, args.blocks // 2), device)
        out.append(f"GroundingDetector, {args.scenes} scenes x 100 000 points, {args.tokens} tokens, 256 queries, MinkResNet-34, 6 layers, "
                   "random weights, device matcher; ms per call (host + device, one stream)")
        out.append(f"  eval forward (predict):        fused {med(ev['fused']):.2f}  per-scene {med(ev['per_scene']):.2f}  "
                   f"blocks fused {[round(x, 2) for x in ev['fused']]} per-scene {[round(x, 2) for x in ev['per_scene']]}")
        out.append(f"  training step (loss+backward): fused {med(tr['fused']):.2f}  per-scene {med(tr['per_scene']):.2f}  "
                   f"blocks fused {[round(x, 2) for x in tr['fused']]} per-scene {[round(x, 2) for x in tr['per_scene']]}")
    text = "\n".join(out) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
