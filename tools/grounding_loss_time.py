#!/usr/bin/env python3
"""Time the grounding loss (proxytransformation_amd/grounding_loss.py) on an MI355X and write the report profiles/grounding_loss.txt
keeps.

Input: the shipped configuration's shapes -- 6 decoder layers, 6 scenes, 256 queries, 77 text tokens of ``max_text_len = 256`` with a
valid prefix per scene, 1 to 4 ground-truth boxes per scene; N(0, 2) scores with ``-inf`` on the masked columns, as
``contrastive_scores`` leaves them.

Two sides, whole calls through Python, HIP events:

* ``hungarian_assign`` (one launch, one copy, one synchronise, scipy on the host), ``grounding_loss`` forward, and forward + backward;
* the torch composition of the reference's lines on the same device and inputs: per layer and scene the three cost matrices with torch
  ops (match_cost.py:227-237, ``cdist``), ``.cpu()``, scipy (hungarian_assigner.py:111-135); per layer the focal loss over
  ``masked_select`` and the four Chamfer terms (chamfer_distance.py:58-63, 160-203), backward through autograd.  The reference's IoU is a
  CUDA extension with no ROCm build, so this side is HANDED THIS PROJECT'S ``box_iou3d``; and it runs WITHOUT the reference's 20 ms sleep
  per (layer, scene) (0.72 s per step at these shapes).

Per side: the median of --blocks blocks of --reps calls after a warm-up block, the sides alternating, with the range of the blocks.

Usage (on a GPU):  python tools/grounding_loss_time.py [--blocks 7] [--reps 10] [--out profiles/grounding_loss.txt]
"""
from __future__ import annotations

import argparse
import math
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F
from scipy.optimize import linear_sum_assignment

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from sparse_conv_time import alternate      # noqa: E402

NL, B, K, T, M = 6, 6, 256, 77, 256
G = (1, 4, 2, 3, 1, 2)
ALPHA, GAMMA, DW = 0.25, 2.0, (0.2, 0.2, 0.2, 0.4)


def euler_zxy(angles):
    c, s = torch.cos(angles), torch.sin(angles)
    one, zero = torch.ones_like(c[..., 0]), torch.zeros_like(c[..., 0])
    rz = torch.stack([c[..., 0], -s[..., 0], zero, s[..., 0], c[..., 0], zero, zero, zero, one], -1).reshape(angles.shape[:-1] + (3, 3))
    rx = torch.stack([one, zero, zero, zero, c[..., 1], -s[..., 1], zero, s[..., 1], c[..., 1]], -1).reshape(angles.shape[:-1] + (3, 3))
    ry = torch.stack([c[..., 2], zero, s[..., 2], zero, one, zero, -s[..., 2], zero, c[..., 2]], -1).reshape(angles.shape[:-1] + (3, 3))
    return rz @ rx @ ry


def corners(bbox):
    signs = torch.tensor([[1, 1, 1], [1, 1, -1], [1, -1, 1], [1, -1, -1], [-1, 1, 1], [-1, 1, -1], [-1, -1, 1], [-1, -1, -1]],
                         dtype=bbox.dtype, device=bbox.device)
    local = signs[None] * (bbox[:, None, 3:6] / 2)
    return bbox[:, None, :3] + torch.matmul(local, euler_zxy(bbox[:, 6:]).transpose(1, 2))


def cd_loss(source, target):
    src, dst = corners(source), corners(target)
    distance = F.l1_loss(src.unsqueeze(2).repeat(1, 1, 8, 1), dst.unsqueeze(1).repeat(1, 8, 1, 1), reduction="none").sum(-1)
    return torch.mean(torch.min(distance, dim=2)[0])


def torch_assign(scores, boxes, mask, gts, pms, iou):
    out = torch.full((NL, B, K), -1, dtype=torch.int32, device=scores.device)
    for l in range(NL):
        for b in range(B):
            idx = torch.nonzero(mask[b]).squeeze(-1)
            p = scores[l, b][:, idx].sigmoid()
            y = pms[b][:, idx]
            neg = -(1 - p + 1e-12).log() * (1 - ALPHA) * p.pow(GAMMA)
            pos = -(p + 1e-12).log() * ALPHA * (1 - p).pow(GAMMA)
            cost = torch.einsum("nc,mc->nm", pos, y) + torch.einsum("nc,mc->nm", neg, 1 - y)
            cost = cost + 2.0 * torch.cdist(boxes[l, b], gts[b], p=1) - 2.0 * iou(boxes[l, b], gts[b])
            cost = torch.nan_to_num(cost.detach().cpu(), nan=100.0, posinf=100.0, neginf=-100.0)
            rows, cols = linear_sum_assignment(cost)
            out[l, b, torch.from_numpy(rows).to(scores.device)] = torch.from_numpy(cols).to(scores.device, torch.int32)
    return out


def torch_loss(scores, boxes, mask, gts, pms, assign):
    text_mask = torch.zeros((B, M), dtype=torch.bool, device=scores.device)
    text_mask[:, :T] = mask
    text_mask = text_mask.unsqueeze(1).repeat(1, K, 1)
    gt_all, pm_all = torch.cat(gts), torch.cat(pms)
    offset = torch.tensor(np.concatenate([[0], np.cumsum(G)[:-1]]), device=scores.device)
    out = []
    for l in range(NL):
        matched = assign[l] >= 0
        rows = (assign[l].long() + offset[:, None])[matched]
        labels = torch.zeros((B, K, M), device=scores.device)
        labels[matched] = pm_all[rows]
        pred, target = torch.masked_select(scores[l], text_mask), torch.masked_select(labels, text_mask)
        p = pred.sigmoid()
        pt = (1 - p) * target + p * (1 - target)
        w = (ALPHA * target + (1 - ALPHA) * (1 - target)) * pt.pow(GAMMA)
        num_pos = sum(min(K, g) for g in G)
        loss_cls = (F.binary_cross_entropy_with_logits(pred, target, reduction="none") * w).sum() / (num_pos + torch.finfo(torch.float32).eps)
        preds, targets = boxes[l][matched], gt_all[rows]
        loss_bbox = DW[0] * cd_loss(torch.cat((preds[:, :3], targets[:, 3:]), -1), targets)
        loss_bbox = loss_bbox + DW[1] * cd_loss(torch.cat((targets[:, :3], preds[:, 3:6], targets[:, 6:]), -1), targets)
        loss_bbox = loss_bbox + DW[2] * cd_loss(torch.cat((targets[:, :6], preds[:, 6:]), -1), targets)
        loss_bbox = loss_bbox + DW[3] * cd_loss(preds, targets)
        out.append((loss_cls, loss_bbox))
    return torch.stack([torch.stack([o[0] for o in out]), torch.stack([o[1] for o in out])])


def spread(values):
    return f"(min {min(values):.1f}, max {max(values):.1f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grounding_loss.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("grounding_loss_time.py measures on a GPU: none found")
    from proxytransformation_amd import grounding_loss as gl
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
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
    scores, boxes, mask, gts, pms = put(scores), put(boxes), put(mask), [put(g) for g in gts], [put(p) for p in pms]
    s_leaf, b_leaf = scores.clone().requires_grad_(), boxes.clone().requires_grad_()
    finite = torch.where(torch.isfinite(scores), scores, torch.zeros_like(scores))      # (the torch side never reads a masked score)
    ts_leaf = finite.clone().requires_grad_()
    up = torch.rand((2, NL), device=dev) + 0.5
    assign = gl.hungarian_assign(scores, boxes, mask, gts, pms)

    def hip_fb():
        return torch.autograd.grad(gl.grounding_loss(s_leaf, b_leaf, mask, gts, pms, assign), [s_leaf, b_leaf], up)

    def torch_fb():
        return torch.autograd.grad(torch_loss(ts_leaf, b_leaf, mask, gts, pms, assign), [ts_leaf, b_leaf], up)

    def no_grad(fn):
        def run():
            with torch.no_grad():
                return fn()
        return run

    rows = [("assign", no_grad(lambda: gl.hungarian_assign(scores, boxes, mask, gts, pms)),
             no_grad(lambda: torch_assign(finite, boxes, mask, gts, pms, gl.box_iou3d))),
            ("loss forward", no_grad(lambda: gl.grounding_loss(scores, boxes, mask, gts, pms, assign)),
             no_grad(lambda: torch_loss(finite, boxes, mask, gts, pms, assign))),
            ("loss forward + backward", hip_fb, torch_fb)]
    lines = [f"grounding loss; {torch.cuda.get_device_name(0)}; {NL} layers, {B} scenes, {K} queries, {T} text tokens of {M}, "
             f"{list(G)} ground-truth boxes per scene",
             f"whole calls through Python, HIP events, median of {args.blocks} blocks of {args.reps} calls after a warm-up block, sides alternating",
             "the torch side is handed this project's box_iou3d (the reference's IoU has no ROCm build) and runs without the reference's "
             "20 ms sleep per (layer, scene)"]
    for name, hip, ref in rows:
        med, t, last = alternate({"hip": hip, "torch": ref}, args.blocks, args.reps)
        a, r = last["hip"], last["torch"]
        if name == "assign":
            note = f"assignments equal at {int((a == r).sum())} of {a.numel()} places"
        elif name == "loss forward":
            note = f"max |hip - torch| / max |torch| {float((a - r).abs().max() / r.abs().max()):.1e}"
        else:
            note = "max |d hip - d torch| / max |d torch|: " + ", ".join(f"{float((x - y).abs().max() / y.abs().max()):.1e}" for x, y in zip(a, r))
        lines.append(f"  {name:24s} hip {med['hip']:9.1f} us {spread(t['hip'])}   torch {med['torch']:9.1f} us {spread(t['torch'])}   torch / hip "
                     f"{med['torch'] / med['hip']:6.2f}" + ("   SLOWER than the torch composition" if med["hip"] > med["torch"] else ""))
        lines.append(f"    {note}")
    text_out = "\n".join(lines) + "\n"
    print(text_out, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text_out)


if __name__ == "__main__":
    main()
