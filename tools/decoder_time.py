#!/usr/bin/env python3
"""Time ``GroundingDecoder.forward`` (proxytransformation_amd/decoder.py: the transformer decoder behind ``QuerySelect``) on an MI355X
and write the report profiles/decoder.txt keeps.

Input: the shipped shape -- six scenes at the row counts ``MinkNeck`` emits (about 3 460 rows each), N(0, 1) features of 256 channels,
77 text tokens with a valid prefix per scene, K = 256 queries, 6 layers, 8 heads, FFN 2048; one regression branch for every layer.

Two sides, whole calls through Python (wrappers, ctypes, ``torch.empty`` of the intermediates), HIP events:

* ``GroundingDecoder.forward`` in eval mode under ``no_grad``;
* the torch composition of the same stage in fp32 on the same device (tests/decoder_util.py ``torch_twin``: ``nn.MultiheadAttention``,
  ``nn.Conv1d`` / ``nn.BatchNorm1d`` / ``nn.LayerNorm`` / ``nn.Linear`` with mmcv's wrapper rules, modules built once).

Per side: the median of --blocks blocks of --reps calls after a warm-up block, the sides alternating, with the range of the blocks.
Then stage by stage: the HIP stage's calls one by one on the chain's own shapes with the achieved TF/s of the GEMM-shaped ones against
the 157 TF fp32 matrix peak, and the torch counterpart of the three heavy ones.  ``--trace`` runs a few forwards and nothing else: the
workload of a ``rocprofv3 --kernel-trace --stats`` run of its own.

Usage (on a GPU):  python tools/decoder_time.py [--blocks 7] [--reps 20] [--out profiles/decoder.txt]
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
from sparse_conv_time import alternate, block_us      # noqa: E402

ROWS = (3461, 3455, 3470, 3448, 3466, 3452)
T, C, K, HEADS, FFN, LAYERS = 77, 256, 256, 8, 2048, 6
PEAK_TF = 157.0


def spread(values):
    return f"(min {min(values):.1f}, max {max(values):.1f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decoder.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("decoder_time.py measures on a GPU: none found")
    from proxytransformation_amd import decoder as dec
    from tests import decoder_util as du
    dev = torch.device("cuda:0")
    m = du.module(C=C, heads=HEADS, ffn=FFN, layers=LAYERS).to(dev)
    branch = du.reg_branches(C, 1)[0].to(dev)
    branches = [branch] * LAYERS
    rng = np.random.default_rng(0)
    tmask = np.ones((len(ROWS), T), bool)
    for b in range(len(ROWS)):
        tmask[b, :int(rng.integers(10, T + 1))] = False
    ops = {k: torch.from_numpy(v).to(dev) for k, v in du.operands(ROWS, K, T, C, 1, tmask).items()}
    twin = du.torch_twin(m, branches, torch.float32, dev)

    def hip():
        with torch.no_grad():
            return m(ops["query"], ops["key"], ops["key"], ops["key_padding_mask"], None, None, ops["query_coords"], ops["key_coords"],
                     ops["pred_bboxes"], ops["text_feats"], ops["text_attention_mask"], branches)

    if args.trace:
        for _ in range(3):
            hip()
        torch.cuda.synchronize()
        return
    B, Lmax, rows = len(ROWS), max(ROWS), sum(ROWS)
    lines = [f"GroundingDecoder({LAYERS} layers, C = {C}, {HEADS} heads, FFN {FFN}) behind QuerySelect; {torch.cuda.get_device_name(0)}; {B} scenes "
             f"of {list(ROWS)} rows (Lmax {Lmax}, {rows} rows in all), T = {T} text tokens, K = {K} queries",
             f"whole calls through Python, HIP events, median of {args.blocks} blocks of {args.reps} calls after a warm-up block, sides alternating"]
    med, t, last = alternate({"hip": hip, "torch": lambda: twin(ops)}, args.blocks, args.reps)
    err = [float((a - b).abs().max() / b.abs().max()) for a, b in zip(last["hip"], last["torch"])]
    lines.append(f"  eval forward   hip {med['hip']:9.1f} us {spread(t['hip'])}   torch {med['torch']:9.1f} us {spread(t['torch'])}   torch / hip "
                 f"{med['torch'] / med['hip']:5.2f}" + ("   SLOWER than the torch composition" if med["hip"] > med["torch"] else ""))
    lines.append(f"    max |hip - torch| / max |torch|: hidden states {err[0]:.1e}, boxes {err[1]:.1e}")

    # stage by stage on the chain's own shapes; flop = the arithmetic of the GEMM-shaped calls (attention: the unmasked keys)
    with torch.no_grad():
        prep = m._prepare(dev)
        g = prep["groups"][0]
        n_g = len(g["ids"])
        a_self, a_scene = (prep["layers"][0][k] for k in ("self_attn", "cross_attn"))
        layer = m.layers[0]
        fc1, fc2 = layer.ffn.layers[0][0], layer.ffn.layers[1]
        query, key, pad = ops["query"], ops["key"], ops["key_padding_mask"]
        key_pos = dec.posembed(ops["key_coords"], prep["cross_pos"])
        query_pos = dec.posembed(ops["pred_bboxes"], prep["self_pos"])
        kv = dec.linear(key, *g["cross_attn"], add=key_pos, add_cols=n_g * C)
        sk, sv = kv[:, :, :C], kv[:, :, n_g * C:(n_g + 1) * C]
        tkv = dec.linear(ops["text_feats"], *g["cross_attn_text"])
        qkv = dec.linear(query, a_self["w"], a_self["b"], add=query_pos, add_cols=2 * C)
        q = dec.linear(query, a_scene["wq"], a_scene["bq"], add=query_pos)
        h = dec.linear(query, fc1.weight, fc1.bias, relu=True)
        wk_all, bk_all = g["cross_attn"]
        gf = lambda n, cin, cout: 2.0 * n * cin * cout / 1e9      # noqa: E731
        parts = [
            ("key_pos: posembed, 3 -> C -> C, once", lambda: dec.posembed(ops["key_coords"], prep["cross_pos"]), gf(B * Lmax, C, C), 1),
            (f"scene k/v of {n_g} layers: linear {C} -> {2 * n_g * C}, once", lambda: dec.linear(key, wk_all, bk_all, add=key_pos, add_cols=n_g * C),
             gf(B * Lmax, C, 2 * n_g * C), 1),
            (f"text k/v of {n_g} layers: linear, once", lambda: dec.linear(ops["text_feats"], *g["cross_attn_text"]), gf(B * T, C, 2 * n_g * C), 1),
            ("query_pos: posembed, 9 -> C -> C", lambda: dec.posembed(ops["pred_bboxes"], prep["self_pos"]), gf(B * K, C, C), LAYERS),
            ("self [q|k|v]: linear C -> 3C", lambda: dec.linear(query, a_self["w"], a_self["b"], add=query_pos, add_cols=2 * C), gf(B * K, C, 3 * C), LAYERS),
            ("self attention, L = K", lambda: dec.attention(qkv[:, :, :C], qkv[:, :, C:2 * C], qkv[:, :, 2 * C:], None, HEADS), 4.0 * B * K * K * C / 1e9,
             LAYERS),
            ("q: linear C -> C (x2: text, scene)", lambda: dec.linear(query, a_scene["wq"], a_scene["bq"], add=query_pos), gf(B * K, C, C), 2 * LAYERS),
            ("text attention, L = T", lambda: dec.attention(q, tkv[:, :, :C], tkv[:, :, n_g * C:(n_g + 1) * C], ops["text_attention_mask"], HEADS),
             4.0 * B * K * T * C / 1e9, LAYERS),
            ("scene attention, L = Lmax", lambda: dec.attention(q, sk, sv, pad, HEADS), 4.0 * K * rows * C / 1e9, LAYERS),
            ("out-projection + identity: linear C -> C (x3)", lambda: dec.linear(q, a_scene["wo"], a_scene["bo"], residual=query), gf(B * K, C, C), 3 * LAYERS),
            ("LayerNorm (x3)", lambda: dec.layer_norm(query, layer.norms[0]), 0.0, 3 * LAYERS),
            ("FFN 1: linear C -> 2048, ReLU", lambda: dec.linear(query, fc1.weight, fc1.bias, relu=True), gf(B * K, C, FFN), LAYERS),
            ("FFN 2 + identity: linear 2048 -> C", lambda: dec.linear(h, fc2.weight, fc2.bias, residual=query), gf(B * K, FFN, C), LAYERS),
            ("LayerNorm + the decoder's norm", lambda: dec.layer_norm(query, layer.norms[3], m.norm), 0.0, LAYERS),
            ("regression branch: 2 x linear C -> C, boxes", lambda: dec.boxes(
                dec.query_select.linear(dec.query_select.linear(query, branch[0].weight, branch[0].bias, None), branch[2].weight, branch[2].bias, None),
                branch[4].weight, branch[4].bias, ops["query_coords"]), 2 * gf(B * K, C, C), LAYERS),
        ]
        lines.append(f"per call of the HIP stage (through its Python wrapper), median of {args.blocks} blocks of {args.reps}; x = calls per forward; "
                     f"TF/s against the {PEAK_TF:.0f} TF fp32 matrix peak:")
        total = 0.0
        for name, fn, gflop, times in parts:
            block_us(fn, args.reps)
            us = sorted(block_us(fn, args.reps)[0] for _ in range(args.blocks))
            mid = us[len(us) // 2]
            total += mid * times
            rate = f"{gflop:7.2f} GFLOP {gflop / mid * 1e3:6.1f} TF/s ({100 * gflop / mid * 1e3 / PEAK_TF:4.1f} %)" if gflop else ""
            lines.append(f"  {name:58s} x{times:<3d}{mid:9.1f} us {spread(us):28s} {rate}")
        lines.append(f"  {'sum over a forward':58s}     {total:9.1f} us")
        # the torch counterpart of the three heavy stages, fp32, same device
        wk, bk = wk_all[:n_g * C], bk_all[:n_g * C]
        wv, bv = wk_all[n_g * C:], bk_all[n_g * C:]
        split = lambda x: x.reshape(B, -1, HEADS, C // HEADS).transpose(1, 2)      # noqa: E731
        skc, svc = sk.contiguous(), sv.contiguous()
        bias = torch.zeros((B, 1, 1, Lmax), device=dev).masked_fill(pad[:, None, None, :], float("-inf"))
        tparts = [(f"scene k/v of {n_g} layers: F.linear(key + key_pos, Wk), F.linear(key, Wv)",
                   lambda: (F.linear(key + key_pos, wk, bk), F.linear(key, wv, bv))),
                  ("scene attention: F.scaled_dot_product_attention with the padding mask",
                   lambda: F.scaled_dot_product_attention(split(q), split(skc), split(svc), attn_mask=bias)),
                  ("FFN: F.linear, relu, F.linear, + identity", lambda: query + F.linear(torch.relu(F.linear(query, fc1.weight, fc1.bias)), fc2.weight, fc2.bias))]
        lines.append("the torch counterpart of the heavy stages (fp32, same device, same protocol):")
        for name, fn in tparts:
            block_us(fn, args.reps)
            us = sorted(block_us(fn, args.reps)[0] for _ in range(args.blocks))
            lines.append(f"  {name:88s} {us[len(us) // 2]:9.1f} us {spread(us)}")
    text_out = "\n".join(lines) + "\n"
    print(text_out, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text_out)


if __name__ == "__main__":
    main()
