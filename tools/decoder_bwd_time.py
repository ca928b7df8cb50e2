#!/usr/bin/env python3
"""Time forward plus backward of the decoder's operators under autograd (proxytransformation_amd/decoder.py with ``differentiable=True``;
csrc/decoder_bwd.hip) on an MI355X and write the report profiles/decoder_bwd.txt keeps.

Shapes: the decoder's at the shipped configuration -- six scenes at the row counts ``MinkNeck`` emits (about 3 460 rows each), 77 text
tokens with a valid prefix per scene, K = 256 queries, C = 256, 8 heads, FFN 2048, the scene keys and values of all six layers hoisted
into one projection (C -> 3072).

Per row two sides, whole calls through Python, HIP events on the stream: the operator with ``differentiable=True`` and
``torch.autograd.grad`` of it against a fixed gradient, and the torch composition of the same operator in fp32 under autograd on the same
device (``F.scaled_dot_product_attention`` with the padding mask as a bias, ``F.linear``, ``F.layer_norm``).  Per side: the median of
--blocks blocks of --reps calls after a warm-up block, the sides alternating, with the range of the blocks; the largest gradient
difference between the sides relative to the torch side's largest value.

Usage (on a GPU):  python tools/decoder_bwd_time.py [--blocks 7] [--reps 20] [--out profiles/decoder_bwd.txt]
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from sparse_conv_time import alternate      # noqa: E402

ROWS = (3461, 3455, 3470, 3448, 3466, 3452)
T, C, K, HEADS, FFN, LAYERS = 77, 256, 256, 8, 2048, 6


def spread(values):
    return f"(min {min(values):.1f}, max {max(values):.1f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decoder_bwd.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("decoder_bwd_time.py measures on a GPU: none found")
    from proxytransformation_amd import decoder as dec
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(0)
    B, Lmax = len(ROWS), max(ROWS)
    rng = np.random.default_rng(0)

    def leaf(*shape, scale=1.0):
        return (torch.randn(shape, generator=g) * scale).to(dev).requires_grad_()

    def const(*shape):
        return torch.randn(shape, generator=g).to(dev)

    pad = torch.zeros((B, Lmax), dtype=torch.bool)
    for b, n in enumerate(ROWS):
        pad[b, n:] = True
    tmask = torch.ones((B, T), dtype=torch.bool)
    for b in range(B):
        tmask[b, :int(rng.integers(10, T + 1))] = False
    pad, tmask = pad.to(dev), tmask.to(dev)
    split = lambda x: x.reshape(B, -1, HEADS, C // HEADS).transpose(1, 2)      # noqa: E731

    def attention_row(L, mask):
        q, k, v, G = leaf(B, K, C), leaf(B, L, C), leaf(B, L, C), const(B, K, C)
        bias = None if mask is None else torch.zeros((B, 1, 1, L), device=dev).masked_fill(mask[:, None, None, :], float("-inf"))
        hip = lambda: torch.autograd.grad(dec.attention(q, k, v, mask, HEADS, differentiable=True), (q, k, v), G)      # noqa: E731
        ref = lambda: torch.autograd.grad(      # noqa: E731
            F.scaled_dot_product_attention(split(q), split(k), split(v), attn_mask=bias).transpose(1, 2).reshape(B, K, C), (q, k, v), G)
        return hip, ref

    def linear_row(n, cin, cout, cols, relu=False):
        x, add, w, b, G = leaf(B, n, cin), leaf(B, n, cin), leaf(cout, cin, scale=cin ** -0.5), leaf(cout, scale=0.1), const(B, n, cout)
        leaves = (x, add, w, b)
        hip = lambda: torch.autograd.grad(dec.linear(x, w, b, add=add, add_cols=cols, relu=relu, differentiable=True), leaves, G)      # noqa: E731

        def ref():
            out = torch.cat([F.linear(x + add, w[:cols], b[:cols]), F.linear(x, w[cols:], b[cols:])], dim=-1)
            return torch.autograd.grad(torch.relu(out) if relu else out, leaves, G)
        return hip, ref

    def ffn_row():
        x, w1, b1, w2, b2, G = leaf(B, K, C), leaf(FFN, C, scale=C ** -0.5), leaf(FFN, scale=0.1), leaf(C, FFN, scale=FFN ** -0.5), \
            leaf(C, scale=0.1), const(B, K, C)
        leaves = (x, w1, b1, w2, b2)
        hip = lambda: torch.autograd.grad(      # noqa: E731
            dec.linear(dec.linear(x, w1, b1, relu=True, differentiable=True), w2, b2, residual=x, differentiable=True), leaves, G)
        ref = lambda: torch.autograd.grad(x + F.linear(torch.relu(F.linear(x, w1, b1)), w2, b2), leaves, G)      # noqa: E731
        return hip, ref

    def ln_row(two):
        x, G, G2 = leaf(B, K, C), const(B, K, C), const(B, K, C)
        p = [leaf(C, scale=0.2) for _ in range(4)]
        with torch.no_grad():
            p[0] += 1.0
            p[2] += 1.0
        leaves = (x, *p) if two else (x, p[0], p[1])
        if two:
            hip = lambda: torch.autograd.grad(dec.layer_norm(x, (p[0], p[1]), (p[2], p[3]), differentiable=True), leaves, (G, G2))      # noqa: E731

            def ref():
                y = F.layer_norm(x, (C,), p[0], p[1], dec.LN_EPS)
                return torch.autograd.grad((y, F.layer_norm(y, (C,), p[2], p[3], dec.LN_EPS)), leaves, (G, G2))
        else:
            hip = lambda: torch.autograd.grad(dec.layer_norm(x, (p[0], p[1]), differentiable=True), leaves, G)      # noqa: E731
            ref = lambda: torch.autograd.grad(F.layer_norm(x, (C,), p[0], p[1], dec.LN_EPS), leaves, G)      # noqa: E731
        return hip, ref

    rows = [("attention self: L = K = 256, no mask", attention_row(K, None)),
            (f"attention text: L = T = {T}, token mask", attention_row(T, tmask)),
            (f"attention scene: L = Lmax = {Lmax}, padding mask", attention_row(Lmax, pad)),
            (f"linear self [q|k|v]: {B * K} x {C} -> {3 * C}, add on 2C", linear_row(K, C, 3 * C, 2 * C)),
            (f"linear scene k/v of {LAYERS} layers: {B * Lmax} x {C} -> {2 * LAYERS * C}, add on half", linear_row(Lmax, C, 2 * LAYERS * C, LAYERS * C)),
            (f"linear FFN pair: {C} -> {FFN} ReLU -> {C} + identity", ffn_row()),
            ("layer_norm: one norm", ln_row(False)),
            ("layer_norm: norms[3] + the decoder's norm, both results used", ln_row(True))]
    lines = [f"decoder operators under autograd, forward + backward; {torch.cuda.get_device_name(0)}; {B} scenes of {list(ROWS)} rows, T = {T}, "
             f"K = {K}, C = {C}, {HEADS} heads",
             f"whole calls through Python, HIP events, median of {args.blocks} blocks of {args.reps} calls after a warm-up block, sides alternating;",
             "torch: the same operator composed in fp32 under autograd on the same device; diff: max |hip - torch| / max |torch| over the gradients"]
    for name, (hip, ref) in rows:
        med, t, last = alternate({"hip": hip, "torch": ref}, args.blocks, args.reps)
        diff = max(float((a - b).abs().max() / b.abs().max()) for a, b in zip(last["hip"], last["torch"]))
        lines.append(f"  {name:72s} hip {med['hip']:9.1f} us {spread(t['hip']):28s} torch {med['torch']:9.1f} us {spread(t['torch']):28s} "
                     f"torch / hip {med['torch'] / med['hip']:5.2f}  diff {diff:.1e}" + ("   BEHIND torch" if med["hip"] > med["torch"] else ""))
    text_out = "\n".join(lines) + "\n"
    print(text_out, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text_out)


if __name__ == "__main__":
    main()
