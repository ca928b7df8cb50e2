#!/usr/bin/env python3
"""Time the decoder's training step and the three operators that close its chain under autograd (``GroundingDecoder(differentiable=True)``,
``posembed`` with batch statistics, ``boxes``, ``contrastive_scores`` of proxytransformation_amd/decoder.py; csrc/decoder_train.hip) on an
MI355X and write the report profiles/decoder_train.txt keeps.

Shapes: the decoder's at the shipped configuration -- six scenes at the row counts ``MinkNeck`` emits (about 3 460 rows each), 77 text
tokens with a valid prefix per scene, K = 256 queries, 6 layers, C = 256, 8 heads, FFN 2048.

Per row two sides, whole calls through Python, HIP events on the stream: the project's side with ``differentiable=True`` and
``torch.autograd.grad`` of it against a fixed gradient, and the same composition in plain torch fp32 under autograd on the same device
(the train-mode twin of tests/decoder_train_util.py for the decoder; ``Conv1d -> BatchNorm1d -> ReLU -> Conv1d``, the Linear with the
decode, the batched product with the mask for the operators).  Per side: the median of --blocks blocks of --reps calls after a warm-up
block, the sides alternating, with the range of the blocks; the largest gradient error of EACH side against the same composition in
float64 on the device, relative to its largest value (torch's fp32 BatchNorm backward on this device is itself percent-level off
float64 over 20 820 rows, so a difference between the sides would say nothing).  Run every invocation under a time limit of its own (``timeout -k 10 600 python tools/decoder_train_time.py``).

Usage (on a GPU):  python tools/decoder_train_time.py [--blocks 7] [--reps 20] [--out profiles/decoder_train.txt]
"""
from __future__ import annotations

import argparse
import math
import os
import sys

import numpy as np
import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from sparse_conv_time import alternate      # noqa: E402
from decoder_bwd_time import C, FFN, HEADS, K, LAYERS, ROWS, T, spread      # noqa: E402

MAX_TEXT = 256


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decoder_train.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("decoder_train_time.py measures on a GPU: none found")
    from proxytransformation_amd import decoder as dec
    from tests import decoder_train_util as tu
    from tests import decoder_util as du
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(0)
    rng = np.random.default_rng(0)
    B, Lmax = len(ROWS), max(ROWS)

    def leaf(*shape, scale=1.0):
        return (torch.randn(shape, generator=g) * scale).to(dev).requires_grad_()

    def const(*shape):
        return torch.randn(shape, generator=g).to(dev)

    pad = torch.zeros((B, Lmax), dtype=torch.bool)
    for b, n in enumerate(ROWS):
        pad[b, n:] = True
    tmask = torch.ones((B, T), dtype=torch.bool)             # True = ignore
    for b in range(B):
        tmask[b, :int(rng.integers(10, T + 1))] = False
    pad, tmask = pad.to(dev), tmask.to(dev)

    def posembed_row(cin, n, padded):
        x = const(B, n, cin) * 3.0
        if padded:
            x = x.masked_fill(pad[:, :, None], 0.0)
        G = const(B, n, C)
        heads = []
        for _ in range(3):
            torch.manual_seed(1)
            heads.append(nn.Sequential(nn.Conv1d(cin, C, 1), nn.BatchNorm1d(C), nn.ReLU(), nn.Conv1d(C, C, 1)).to(dev).train())
        mine, ref, ref64 = heads
        ref64.double()
        xt = x.transpose(1, 2).contiguous()
        hip = lambda: torch.autograd.grad(dec.posembed(x, mine, differentiable=True), list(mine.parameters()), G)      # noqa: E731
        tor = lambda: torch.autograd.grad(ref(xt).transpose(1, 2), list(ref.parameters()), G)      # noqa: E731
        f64 = lambda: torch.autograd.grad(ref64(xt.double()).transpose(1, 2), list(ref64.parameters()), G.double())      # noqa: E731
        return hip, tor, (1,), f64                            # the first layer's bias is zero in exact arithmetic: left out

    def boxes_row():
        h, w, b, coords, G = leaf(B, K, C), leaf(9, C, scale=C ** -0.5), leaf(9, scale=0.1), const(B, K, 3), const(B, K, 9)
        with torch.no_grad():
            b[3:6] -= 3.9
        leaves = (h, w, b)
        hip = lambda: torch.autograd.grad(dec.boxes(h, w, b, coords, differentiable=True), leaves, G)      # noqa: E731

        def tor():
            p = h @ w.T + b
            return torch.autograd.grad(torch.cat([p[..., :3] + coords, torch.exp(p[..., 3:6]).clamp(min=2e-2), p[..., 6:]], -1), leaves, G)

        def f64():
            h6, w6, b6 = (a.detach().double().requires_grad_() for a in leaves)
            p = h6 @ w6.T + b6
            out = torch.cat([p[..., :3] + coords.double(), torch.exp(p[..., 3:6]).clamp(min=2e-2), p[..., 6:]], -1)
            return torch.autograd.grad(out, (h6, w6, b6), G.double())
        return hip, tor, (), f64

    def scores_row():
        hs, text, bias = leaf(LAYERS, B, K, C), leaf(B, T, C), leaf(1)
        keep = ~tmask
        G = torch.where(keep[None, :, None, :].expand(LAYERS, B, K, T), const(LAYERS, B, K, T), torch.zeros((), device=dev))
        Gfull = torch.zeros((LAYERS, B, K, MAX_TEXT), device=dev)
        Gfull[..., :T] = G
        leaves = (hs, text, bias)
        hip = lambda: torch.autograd.grad(dec.contrastive_scores(hs, text, keep, bias, True, MAX_TEXT, differentiable=True), leaves, Gfull)      # noqa: E731

        def tor():
            s = hs @ text.transpose(1, 2)[None] / math.sqrt(C) + bias
            s = s.masked_fill(~keep[None, :, None, :], float("-inf"))
            out = torch.full((LAYERS, B, K, MAX_TEXT), float("-inf"), device=dev)
            out = torch.cat([s, out[..., T:]], -1)
            return torch.autograd.grad(out, leaves, Gfull)

        def f64():
            h6, t6, b6 = (a.detach().double().requires_grad_() for a in leaves)
            s = (h6 @ t6.transpose(1, 2)[None] / math.sqrt(C) + b6).masked_fill(~keep[None, :, None, :], 0.0)
            return torch.autograd.grad(s, (h6, t6, b6), G.double())
        return hip, tor, (), f64

    def decoder_row():
        cfg = dict(C=C, heads=HEADS, ffn=FFN, layers=LAYERS)
        m = du.module(**cfg, differentiable=True).train()
        branches = du.reg_branches(C, LAYERS).train()
        ops = du.operands(ROWS, K, T, C, 5, tmask.cpu().numpy())
        t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in ops.items()}
        for k in ("query", "key", "text_feats"):
            t[k].requires_grad_()
        run, named, _ = tu.train_twin(m, branches, torch.float32, dev)
        import copy
        md, bd = copy.deepcopy(m).to(dev).train(), copy.deepcopy(branches).to(dev).train()
        G = (const(LAYERS, B, K, C), const(LAYERS, B, K, 9))
        names = sorted(named)
        mine = dict(md.named_parameters())
        mine.update({f"reg.{lid}.{n}": p for lid, br in enumerate(bd) for n, p in br.named_parameters()})
        inputs = [t["query"], t["key"], t["text_feats"]]

        def hip():
            out = md(t["query"], t["key"], t["key"], t["key_padding_mask"], None, None, t["query_coords"], t["key_coords"], t["pred_bboxes"],
                     t["text_feats"], t["text_attention_mask"], bd)
            return torch.autograd.grad(out, inputs + [mine[n] for n in names], G)

        def tor():
            return torch.autograd.grad(run(t)[0], inputs + [named[n] for n in names], G)
        zero = tuple(3 + names.index(n) for n in tu.ZERO_LEAVES)
        run64, named64, _ = tu.train_twin(m, branches, torch.float64, dev)
        t64 = {k: (v.detach().double().requires_grad_(v.requires_grad) if v.is_floating_point() else v) for k, v in t.items()}

        def f64():
            return torch.autograd.grad(run64(t64)[0], [t64["query"], t64["key"], t64["text_feats"]] + [named64[n] for n in names],
                                       tuple(a.double() for a in G))
        return hip, tor, zero, f64

    rows = [(f"posembed cross: {B * Lmax} x 3 -> {C}, padded rows as zeros", posembed_row(3, Lmax, True)),
            (f"posembed self: {B * K} x 9 -> {C}", posembed_row(9, K, False)),
            (f"boxes: {B * K} x {C} -> 9 and the decode", boxes_row()),
            (f"contrastive_scores: {LAYERS} x {B} x {K} x {C} . {T} tokens -> {MAX_TEXT}", scores_row()),
            (f"decoder training step: {LAYERS} layers, FFN {FFN}, forward + backward of every parameter and input", decoder_row())]
    lines = [f"training through the decoder, forward + backward; {torch.cuda.get_device_name(0)}; {B} scenes of {list(ROWS)} rows, T = {T}, "
             f"K = {K}, C = {C}, {HEADS} heads, {LAYERS} layers",
             f"whole calls through Python, HIP events, median of {args.blocks} blocks of {args.reps} calls after a warm-up block, sides alternating;",
             "torch: the same composition in fp32 under autograd on the same device; err: the largest max |side - float64| / max |float64| over",
             "the gradients, float64 being the same composition in float64 on the device (the gradients that are zero in exact arithmetic left out)"]
    for name, (hip, tor, skip, f64) in rows:
        med, t, last = alternate({"hip": hip, "torch": tor}, args.blocks, args.reps)
        ref = f64()
        err = {k: max(float((a.double() - b).abs().max() / b.abs().max()) for i, (a, b) in enumerate(zip(last[k], ref)) if i not in skip)
               for k in ("hip", "torch")}
        lines.append(f"  {name:96s} hip {med['hip']:9.1f} us {spread(t['hip']):30s} torch {med['torch']:9.1f} us {spread(t['torch']):30s} "
                     f"torch / hip {med['torch'] / med['hip']:5.2f}  err hip {err['hip']:.1e} torch {err['torch']:.1e}"
                     + ("   BEHIND torch" if med["hip"] > med["torch"] else ""))
    text_out = "\n".join(lines) + "\n"
    print(text_out, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text_out)


if __name__ == "__main__":
    main()
