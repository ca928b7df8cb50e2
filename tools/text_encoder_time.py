#!/usr/bin/env python3
"""Time ``ClipTextEncoder.forward`` (proxytransformation_amd/text_encoder.py: the CLIP text encoder in front of ``text_feat_map``) on an
MI355X and write the report profiles/text_encoder.txt keeps.

Input: the shipped shape -- 6 texts x 77 tokens, 12 layers of width 768 (12 heads of 64), MLP 3072, vocabulary 49408; the seeded weights
of tests/text_encoder_util.py; a valid prefix of 8 to 77 tokens per text.

Two sides, whole calls through Python (ctypes, ``torch.empty`` of the intermediates), HIP events:

* ``ClipTextEncoder.forward``;
* the torch fp32 composition of the same stage on the same device (tests/text_encoder_util.py ``torch_forward``:
  ``F.layer_norm``, ``F.linear``, ``F.scaled_dot_product_attention`` under the causal and padding mask), under ``no_grad``.

Per side: the median of --blocks blocks of --reps calls after a warm-up block, the sides alternating, with the range of the blocks.
The floor both are reported against is the weight stream: the layers' fp32 weights (340 MB at the shipped shape, more than the cache
holds) at 4 TB/s.  Then launch by launch on the chain's own shapes: each entry point of csrc/text_encoder.hip through ctypes and its
torch counterpart, same protocol, with the achieved TF/s of the GEMM-shaped ones against the 157 TF fp32 matrix peak.  ``--trace`` runs
a few forwards and nothing else: the workload of a ``rocprofv3 --kernel-trace --stats`` run of its own.

Usage (on a GPU):  python tools/text_encoder_time.py [--blocks 7] [--reps 10] [--out profiles/text_encoder.txt]
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

B, T, C, H, I, LAYERS, VOCAB = 6, 77, 768, 12, 3072, 12, 49408
PEAK_TF, PEAK_TBS = 157.0, 4.0


def spread(values):
    return f"(min {min(values):.1f}, max {max(values):.1f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "text_encoder.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("text_encoder_time.py measures on a GPU: none found")
    from proxytransformation_amd import _abi
    from tests import text_encoder_util as U
    dev = torch.device("cuda:0")
    params = U.make_params(C, I, LAYERS, vocab=VOCAB)
    enc = U.build_encoder(C, H, I, LAYERS, vocab=VOCAB, params=params).to(dev)
    tp = {k: torch.from_numpy(v).to(dev) for k, v in params.items()}
    rng = np.random.default_rng(0)
    ids_np = U.make_ids(B, T, vocab=VOCAB)
    mask_np = np.zeros((B, T), bool)
    for b in range(B):
        mask_np[b, :int(rng.integers(8, T + 1))] = True
    ids, mask = torch.from_numpy(ids_np).to(dev), torch.from_numpy(mask_np).to(dev)

    def hip():
        return enc(ids, mask)

    def twin():
        with torch.no_grad():
            return U.torch_forward(tp, ids, mask, H)

    if args.trace:
        for _ in range(3):
            hip()
        torch.cuda.synchronize()
        return
    n = B * T
    layer_bytes = 4.0 * LAYERS * (4 * C * C + 2 * C * I + 9 * C + I)
    floor_us = layer_bytes / (PEAK_TBS * 1e12) * 1e6
    gflop_fwd = LAYERS * 2.0 * n * (4 * C * C + 2 * C * I) / 1e9
    lines = [f"ClipTextEncoder({LAYERS} layers, C = {C}, {H} heads, MLP {I}, vocabulary {VOCAB}); {torch.cuda.get_device_name(0)}; {B} texts x {T} "
             f"tokens ({n} rows), valid prefixes {mask_np.sum(1).tolist()}",
             f"whole calls through Python, HIP events, median of {args.blocks} blocks of {args.reps} calls after a warm-up block, sides alternating",
             f"floor: the layers' weights, {layer_bytes / 1e6:.0f} MB of fp32 per forward at {PEAK_TBS:.0f} TB/s = {floor_us:.0f} us; the GEMMs are "
             f"{gflop_fwd:.1f} GFLOP = {gflop_fwd / PEAK_TF * 1e3:.0f} us at the {PEAK_TF:.0f} TF fp32 matrix peak"]
    med, t, last = alternate({"hip": hip, "torch": twin}, args.blocks, args.reps)
    valid = mask_np[:, :, None].repeat(C, 2)
    a, b = last["hip"].cpu().numpy(), last["torch"].cpu().numpy()
    err = float(np.abs(a - b)[valid].max() / np.abs(b[valid]).max())
    lines.append(f"  forward        hip {med['hip']:9.1f} us {spread(t['hip'])}   torch {med['torch']:9.1f} us {spread(t['torch'])}   torch / hip "
                 f"{med['torch'] / med['hip']:5.2f}" + ("   SLOWER than the torch composition" if med["hip"] > med["torch"] else ""))
    lines.append(f"    hip / floor {med['hip'] / floor_us:6.1f}   torch / floor {med['torch'] / floor_us:6.1f}   "
                 f"hip {gflop_fwd / med['hip'] * 1e3:5.1f} TF/s   torch {gflop_fwd / med['torch'] * 1e3:5.1f} TF/s over the whole call")
    lines.append(f"    max |hip - torch| / max |torch| over the rows of valid tokens: {err:.1e}")

    # launch by launch on the chain's own shapes
    lib, st = _abi.lib(), torch.cuda.current_stream(dev).cuda_stream
    with torch.no_grad():
        prep = enc._prepare(dev)
        L = prep["layers"][0]
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)      # noqa: E731
        x = hip().reshape(n, C).contiguous()                 # O(1) rows
        qkv, attn, hid, out, stats = new(n, 3 * C), new(n, C), new(n, I), new(n, C), new(n, 2)
        nbytes = int(lib.ptx_txt_linear_workspace_bytes(n, I, C))
        ws = torch.empty((nbytes // 4,), dtype=torch.float32, device=dev)
        p = lambda t_: t_.data_ptr()      # noqa: E731
        lib.ptx_txt_ln_linear(p(x), n, p(L["ln1"][0]), p(L["ln1"][1]), 1e-5, p(L["wqkv"]), p(L["bqkv"]), C, 3 * C, 0, p(qkv), p(stats), st)
        lib.ptx_txt_attention(p(qkv), p(mask), B, T, H, p(attn), st)
        lib.ptx_txt_ln_linear(p(x), n, p(L["ln2"][0]), p(L["ln2"][1]), 1e-5, p(L["w1"]), p(L["b1"]), C, I, 1, p(hid), p(stats), st)
        pre = "text_model.encoder.layers.0."
        W = lambda name: tp[pre + name]      # noqa: E731
        wqkv_t, bqkv_t = L["wqkv"], L["bqkv"]
        allow = torch.ones((T, T), dtype=torch.bool, device=dev).tril()[None, None] & mask[:, None, None, :]
        heads = lambda z: z.view(B, T, H, 64).transpose(1, 2)      # noqa: E731
        gf = lambda cin, cout: 2.0 * n * cin * cout / 1e9      # noqa: E731
        attn_gf = 4.0 * B * H * 64 * sum(int(mask_np[b_, :t_ + 1].sum()) for b_ in range(B) for t_ in range(T)) / 1e9
        parts = [
            ("embed: gather + positions",
             lambda: lib.ptx_txt_embed(p(ids), B, T, p(prep["tok"]), p(prep["pos"]), VOCAB, 77, C, p(out), st),
             lambda: tp["text_model.embeddings.token_embedding.weight"][ids] + tp["text_model.embeddings.position_embedding.weight"][:T], 0.0, 1),
            ("LN1 -> [q|k|v]: C -> 3C (statistics + GEMM)",
             lambda: lib.ptx_txt_ln_linear(p(x), n, p(L["ln1"][0]), p(L["ln1"][1]), 1e-5, p(L["wqkv"]), p(L["bqkv"]), C, 3 * C, 0, p(qkv), p(stats), st),
             lambda: F.linear(F.layer_norm(x, (C,), L["ln1"][0], L["ln1"][1], 1e-5), wqkv_t, bqkv_t), gf(C, 3 * C), LAYERS),
            ("causal attention",
             lambda: lib.ptx_txt_attention(p(qkv), p(mask), B, T, H, p(attn), st),
             lambda: F.scaled_dot_product_attention(heads(qkv[:, :C]), heads(qkv[:, C:2 * C]), heads(qkv[:, 2 * C:]), attn_mask=allow), attn_gf, LAYERS),
            ("out_proj + residual: C -> C",
             lambda: lib.ptx_txt_linear(p(attn), n, p(L["wo"]), p(L["bo"]), C, C, p(x), p(out), p(ws), nbytes, st),
             lambda: x + F.linear(attn, L["wo"], L["bo"]), gf(C, C), LAYERS),
            ("LN2 -> fc1 -> quick-GELU: C -> I (same)",
             lambda: lib.ptx_txt_ln_linear(p(x), n, p(L["ln2"][0]), p(L["ln2"][1]), 1e-5, p(L["w1"]), p(L["b1"]), C, I, 1, p(hid), p(stats), st),
             lambda: (lambda h_: h_ * torch.sigmoid(1.702 * h_))(F.linear(F.layer_norm(x, (C,), L["ln2"][0], L["ln2"][1], 1e-5), L["w1"], L["b1"])),
             gf(C, I), LAYERS),
            ("fc2 + residual: I -> C (4 slices + their sum)",
             lambda: lib.ptx_txt_linear(p(hid), n, p(L["w2"]), p(L["b2"]), I, C, p(x), p(out), p(ws), nbytes, st),
             lambda: x + F.linear(hid, L["w2"], L["b2"]), gf(I, C), LAYERS),
            ("final LayerNorm",
             lambda: lib.ptx_txt_ln(p(x), n, C, p(prep["fw"]), p(prep["fb"]), 1e-5, p(out), st),
             lambda: F.layer_norm(x, (C,), prep["fw"], prep["fb"], 1e-5), 0.0, 1),
        ]
        lines.append(f"launch by launch (hip: the entry point through ctypes; torch: its fp32 counterpart), median of {args.blocks} blocks of "
                     f"{args.reps}, sides alternating; x = calls per forward; one layer's weights, so they stay in the cache here; TF/s of the hip side "
                     f"against the {PEAK_TF:.0f} TF fp32 matrix peak:")
        total = {"hip": 0.0, "torch": 0.0}
        for name, hfn, tfn, gflop, times in parts:
            m2, t2, _ = alternate({"hip": hfn, "torch": tfn}, args.blocks, args.reps * 5)
            for k in total:
                total[k] += m2[k] * times
            rate = f"{gflop:6.2f} GFLOP {gflop / m2['hip'] * 1e3:6.1f} TF/s ({100 * gflop / m2['hip'] * 1e3 / PEAK_TF:4.1f} %)" if gflop else ""
            flag = "  BEHIND" if m2["hip"] > m2["torch"] else ""
            lines.append(f"  {name:46s} x{times:<3d} hip {m2['hip']:8.1f} us {spread(t2['hip']):24s} torch {m2['torch']:8.1f} us "
                         f"{spread(t2['torch']):24s} torch / hip {m2['torch'] / m2['hip']:5.2f}{flag}  {rate}")
        lines.append(f"  {'sum over a forward':46s}      hip {total['hip']:8.1f} us {'':24s} torch {total['torch']:8.1f} us")
    text_out = "\n".join(lines) + "\n"
    print(text_out, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text_out)


if __name__ == "__main__":
    main()
