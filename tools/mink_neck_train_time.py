#!/usr/bin/env python3
"""Time one training step -- forward plus backward, BatchNorms in training mode -- of the shipped ``MinkNeck(differentiable=True)``
([128, 256, 512, 1024] -> 256, one class, pts_prune_threshold 1000) on an MI355X, by stage and as a whole, and write the report
profiles/mink_neck_train.txt keeps.  The input is tools/mink_neck_time.py's: six room clouds through ``MinkResNet(34, 3)``, every level's
features concatenated with as many random channels.

Two sides, whole calls through Python, HIP events:

* the training chain's stages one by one, each on the HIP chain's own inputs of that stage, forward and backward
  (``torch.autograd.grad`` of the stage's result with respect to its inputs and parameters, with a fixed random ``g``) -- generative
  transposed convolution + BatchNorm + ELU, the 3x3x3 convolution (+ kernel map) + BatchNorm + ELU, union add, prune scores (no
  gradient: forward only), top-k prune, the output block (+ kernel map), the head -- summed over the levels;
* the torch composition of the same stage on the same rows (tools/mink_neck_time.py's, with ``F.batch_norm(training=True)`` + ``F.elu``
  behind the raw products and autograd's own backward), handed OUR neighbour tables.

Per stage and side: the median of --blocks blocks of --reps calls after a warm-up block, the sides alternating.  Then the whole
training step (``forward`` + ``loss.backward()``, median of --blocks calls) and, for comparison with profiles/mink_neck.txt, the eval
forward of the same module (the folded route).

Usage (on a GPU):  python tools/mink_neck_train_time.py [--blocks 5] [--reps 4] [--out profiles/mink_neck_train.txt]
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
from mink_neck_time import K, OUT, WIDTHS, t_head, t_scores, t_topk, t_union      # noqa: E402
from sparse_conv_time import B, N, VOXEL, alternate, offset_lists, room_points, torch_layer      # noqa: E402


def t_block(z, bn):
    return F.elu(F.batch_norm(z, bn.running_mean, bn.running_var, bn.weight, bn.bias, True, bn.momentum, bn.eps))


def grads_of(out, leaves, g):
    return torch.autograd.grad(out, leaves, g)


def whole(fn, blocks):
    t = []
    for blk in range(blocks + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        r = fn()
        b.record()
        b.synchronize()
        if blk:
            t.append(a.elapsed_time(b))
    return t, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mink_neck_train.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mink_neck_train_time.py measures on a GPU: none found")
    from bench import build_module
    from proxytransformation_amd import MinkNeck, MinkResNet, neck, sparse
    from proxytransformation_amd.backbone import SparseLevel
    from proxytransformation_amd.synth import CONFIGS
    dev = torch.device("cuda:0")
    mod, _ = build_module(CONFIGS["cfg4_room"], dev)
    torch.manual_seed(0)
    net = MinkResNet(34, 3).to(dev).eval()
    m = MinkNeck(1, list(WIDTHS), OUT, VOXEL, K, differentiable=True).to(dev).train()
    m.init_weights()
    gen = torch.Generator(device=dev).manual_seed(3)
    stages = ["generative conv + BN", "map + conv k3 + BN (up)", "union add", "prune scores (fwd only)", "top-k prune", "map + conv k3 + BN (out)",
              "head"]
    hip = {k: 0.0 for k in stages}
    tor = {k: 0.0 for k in stages}
    diff = {k: 0.0 for k in stages}
    rnd = lambda t: torch.randn(t.shape, generator=gen, device=dev)      # noqa: E731
    leaf = lambda t: t.detach().clone().requires_grad_()                  # noqa: E731
    with torch.no_grad():
        pts = [torch.from_numpy(room_points(900 + b, N)).to(dev) for b in range(B)]
        coords, feats3, ends = mod.quantize(pts, VOXEL, return_scene_rows=True)
        levels = [SparseLevel(torch.cat([lv.feats, torch.randn(lv.feats.shape, generator=gen, device=dev)], 1).contiguous(), lv.coords,
                              lv.scene_rows, lv.tensor_stride) for lv in net(coords, ends, feats3.contiguous())]

    def both(name, hip_fn, torch_fn):
        """Each side returns (result, *gradients); the float tensors of the two sides are compared."""
        med, _, last = alternate({"hip": hip_fn, "torch": torch_fn}, args.blocks, args.reps)
        hip[name] += med["hip"]
        tor[name] += med["torch"]
        flo = lambda r: [t for t in (r if isinstance(r, tuple) else (r,)) if isinstance(t, torch.Tensor) and t.is_floating_point()]  # noqa: E731
        for h, t in zip(flo(last["hip"]), flo(last["torch"])):
            if h.numel() == t.numel() and h.numel():
                diff[name] = max(diff[name], float((h.detach() - t.detach().reshape(h.shape)).abs().max() / t.detach().abs().max().clamp(min=1e-30)))
            else:
                diff[name] = float("nan")
        return last["hip"]

    def conv_stage(name, conv, bn, x, c, e, ts):
        """conv k3 (+ its kernel map) -> training BatchNorm + ELU, forward and backward; returns the result, detached."""
        lists = offset_lists(sparse.kernel_map(c, e, ts, 3, 1).nbr)
        xl = leaf(x)
        with torch.no_grad():
            g = rnd(bn(conv(x, sparse.kernel_map(c, e, ts, 3, 1)), elu=True))
        par = [conv.kernel, bn.bn.weight, bn.bn.bias]

        def h():
            y = bn(conv(xl, sparse.kernel_map(c, e, ts, 3, 1)), elu=True)
            return (y.detach(),) + grads_of(y, [xl] + par, g)

        def t():
            y = t_block(torch_layer(xl, conv.kernel, lists, c.shape[0]), bn.bn)
            return (y.detach(),) + grads_of(y, [xl] + par, g)

        return both(name, h, t)[0]

    top = len(levels) - 1
    c, e, ts, x = levels[top].coords, list(levels[top].scene_rows), levels[top].tensor_stride, levels[top].feats
    score = None
    rows = []
    for i in range(top, -1, -1):
        if i < top:
            up = getattr(m, f"up_block_{i + 1}")
            xl = leaf(x)
            with torch.no_grad():
                g0 = rnd(up[0](c, e, ts, x)[2])
            par = [up[0].kernel, up[1].bn.weight, up[1].bn.bias]

            def h_gen():
                gc, ge, z = up[0](c, e, ts, xl)
                y = up[1](z, elu=True)
                return (y.detach(),) + grads_of(y, [xl] + par, g0) + (gc, ge)

            def t_gen():
                z = torch.stack([xl @ up[0].kernel[j] for j in range(8)], 1).reshape(-1, up[0].kernel.shape[2])
                y = t_block(z, up[1].bn)
                return (y.detach(),) + grads_of(y, [xl] + par, g0)

            r = both(stages[0], h_gen, t_gen)
            g, gc, ge = r[0], r[-2], r[-1]
            g2 = conv_stage(stages[1], up[3], up[4], g, gc, ge, ts // 2)
            lv = levels[i]
            al, bl = leaf(lv.feats), leaf(g2)
            with torch.no_grad():
                gu = rnd(neck.union_add(lv.coords, lv.scene_rows, lv.feats, gc, ge, g2, ts // 2)[2])

            def h_union():
                uc, ue, u = neck.union_add(lv.coords, lv.scene_rows, al, gc, ge, bl, ts // 2, differentiable=True)
                return (u.detach(),) + grads_of(u, [al, bl], gu) + (uc, ue)

            def t_un():
                uc, u = t_union(lv.coords, lv.scene_rows, al, gc, ge, bl)
                return (u.detach(),) + grads_of(u, [al, bl], gu)

            r = both(stages[2], h_union, t_un)
            u, uc, ue = r[0], r[-2], r[-1]
            with torch.no_grad():
                q = both(stages[3], lambda: neck.prune_scores(uc, c, e, ts, score), lambda: t_scores(uc, c, score, ts))
            rows.append((int(gc.shape[0]), int(uc.shape[0])))
            ul = leaf(u)
            with torch.no_grad():
                gp = rnd(neck.topk_prune(q, uc, ue, u, K)[2])

            def h_prune():
                pc, pe, pf, _ = neck.topk_prune(q, uc, ue, ul, K, differentiable=True)
                return (pf.detach(),) + grads_of(pf, [ul], gp) + (pc, pe)

            def t_prune():
                _, pf = t_topk(q, uc, ue, ul, K)
                return (pf.detach(),) + grads_of(pf, [ul], gp)

            r = both(stages[4], h_prune, t_prune)
            x, c, e = r[0], r[-2], r[-1]
            ts //= 2
        ob = getattr(m, f"out_block_{i}")
        out = conv_stage(stages[5], ob[0], ob[1], x, c, e, ts)
        ol = leaf(out)
        w, bias = m.conv_cls.kernel, m.conv_cls.bias
        with torch.no_grad():
            gh = rnd(neck.neck_head(out, w, bias)[0])

        def h_head():
            cls, sc = neck.neck_head(ol, w, bias, differentiable=True)
            return (cls.detach(),) + grads_of(cls, [ol, w, bias], gh) + (sc,)

        def t_hd():
            cls, sc = t_head(ol, w[0], bias)
            return (cls.detach(),) + grads_of(cls, [ol, w, bias], gh)

        score = both(stages[6], h_head, t_hd)[-1]

    lv_grad = [SparseLevel(leaf(lv.feats), lv.coords, lv.scene_rows, lv.tensor_stride) for lv in levels]
    with torch.no_grad():
        f0, s0, _ = m(levels, B)
    gf, gs = [rnd(f) for f in f0], [rnd(s) for s in s0]

    def step():
        for p in list(m.parameters()) + [lv.feats for lv in lv_grad]:
            p.grad = None
        feats, scores, _ = m(lv_grad, B)
        loss = sum((f * g).sum() for f, g in zip(feats, gf)) + sum((s * g).sum() for s, g in zip(scores, gs))
        loss.backward()
        return feats

    t_step, feats = whole(step, args.blocks)
    with torch.no_grad():
        t_fwd, _ = whole(lambda: m(levels, B), args.blocks)
        m.eval()
        t_eval, _ = whole(lambda: m(levels, B), args.blocks)
    lines = [f"MinkNeck({list(WIDTHS)} -> {OUT}, 1 class, pts_prune_threshold {K}, differentiable=True) training step (BatchNorms in training mode); "
             f"{torch.cuda.get_device_name(0)}; {B} room clouds x {N} points at {VOXEL * 100:g} cm -> levels of "
             f"{[int(lv.feats.shape[0]) for lv in levels]} rows; per step (generated rows, union rows): {rows}; output rows per scene: "
             f"{[int(f.shape[0]) for f in feats]}",
             f"per stage FORWARD + BACKWARD, summed over the levels, median of {args.blocks} blocks of {args.reps} calls, sides alternating; whole "
             f"calls through Python; the torch side is handed the neighbour tables (kernel maps are on the HIP side only)"]
    for k in stages:
        lines.append(f"  {k:26s} hip {hip[k]:9.1f} us   torch {tor[k]:9.1f} us   torch / hip {tor[k] / hip[k]:5.2f}" +
                     f"   max |hip - torch| / max |torch| {diff[k]:.1e}" + ("   SLOWER than the torch composition" if hip[k] > tor[k] else ""))
    lines.append(f"  {'sum of the stages':26s} hip {sum(hip.values()):9.1f} us   torch {sum(tor.values()):9.1f} us   torch / hip "
                 f"{sum(tor.values()) / sum(hip.values()):5.2f}")
    med = statistics.median
    lines.append(f"whole training step, forward + backward (one call each, median of {args.blocks}): {med(t_step):.3f} ms (min {min(t_step):.3f}, "
                 f"max {max(t_step):.3f}); its forward alone under no_grad: {med(t_fwd):.3f} ms")
    lines.append(f"eval forward of the same module (folded route, median of {args.blocks}): {med(t_eval):.3f} ms (min {min(t_eval):.3f}, "
                 f"max {max(t_eval):.3f})")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
