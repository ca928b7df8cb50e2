#!/usr/bin/env python3
"""Time ``QuerySelect.forward`` (proxytransformation_amd/query_select.py: the detector's ``pre_decoder`` behind the neck) on an MI355X and
write the report profiles/query_select.txt keeps.

Input: six scenes at the row counts ``MinkNeck`` emits for the shipped configuration (profiles/mink_neck.txt: three pruned levels of
1000 rows plus the coarsest level, about 450 rows, per scene), N(0, 1) features of 256 channels, 77 text tokens with a valid prefix per
scene, ``num_queries = 256``; the regression branch with N(0, 2 / C) weights.

Two sides, whole calls through Python (wrappers, ctypes, ``torch.empty`` of the outputs), HIP events:

* ``QuerySelect.forward`` in eval mode under ``no_grad``, and the training step -- ``QuerySelect(differentiable=True).forward`` plus the
  backward of a gradient on ``query`` and ``feats``;
* the torch composition of the same stage on the same inputs in the reference's order of operations (sparse_featfusion_grounder_preshape.py:
  498-580): ``cat`` with the coordinates, zero padding, ``stack``, ``ContrastiveEmbed`` (matmul, scale, bias, two ``masked_fill_``, the
  ``-inf`` tensor of ``max_text_len`` columns), ``max``, ``topk``, the regression branch over ALL rows, the decode, three ``gather``;
  its training step backpropagates the same two gradients through autograd.

Per side: the median of --blocks blocks of --reps calls after a warm-up block, the sides alternating, with the range of the blocks.
Then the HIP stage's calls one by one on the chain's own operands (the per-kernel breakdown; each is one launch).

Usage (on a GPU):  python tools/query_select_time.py [--blocks 7] [--reps 20] [--out profiles/query_select.txt]
"""
from __future__ import annotations

import argparse
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from sparse_conv_time import alternate, block_us      # noqa: E402

ROWS = (3461, 3455, 3470, 3448, 3466, 3452)            # 3 x 1000 + the coarsest level of each scene
T, C, QUERIES, MAX_TEXT = 77, 256, 256, 256


def torch_stage(feats_list, xyz_list, text_feats, text_token_mask, cls_bias, reg, num_queries):
    """The stage as a user writes it in torch today, in the reference's order."""
    joined = [torch.cat((f, p), dim=-1) for f, p in zip(feats_list, xyz_list)]
    longest = max(j.size(0) for j in joined)
    shortest = min(j.size(0) for j in joined)
    padded, valid = [], []
    for j in joined:
        if longest > j.size(0):
            j = torch.cat([j, torch.zeros(longest - j.size(0), j.size(1), device=j.device)], dim=0)
        padded.append(j)
    for f in feats_list:
        v = torch.zeros(longest, dtype=torch.bool, device=f.device)
        v[:f.size(0)] = 1
        valid.append(v)
    both, valid = torch.stack(padded), torch.stack(valid)
    feats, coords = both[..., :-3], both[..., -3:]
    res = feats @ text_feats.transpose(-1, -2)
    res = res / math.sqrt(feats.shape[-1])
    res = res + cls_bias
    res.masked_fill_(~text_token_mask[:, None, :], float("-inf"))
    res.masked_fill_(~valid[:, :, None], float("-inf"))
    full = torch.full((*res.shape[:-1], MAX_TEXT), float("-inf"), device=res.device)
    full[..., :res.shape[-1]] = res
    k = min(num_queries, shortest)
    index = torch.topk(full.max(-1)[0], k=k, dim=1)[1]
    p = reg(feats)
    boxes = torch.cat((p[..., :3] + coords, torch.exp(p[..., 3:6]).clamp(min=2e-2), p[..., 6:]), dim=-1)
    take = lambda t: torch.gather(t, 1, index.unsqueeze(-1).repeat(1, 1, t.size(-1)))      # noqa: E731
    return dict(query=take(feats), feats=feats, feats_attention_mask=~valid, query_coords=take(coords), feats_coords=coords,
                pred_bboxes=take(boxes).detach().clone(), text_feats=text_feats, text_attention_mask=~text_token_mask), index


def spread(values):
    return f"(min {min(values):.1f}, max {max(values):.1f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "query_select.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("query_select_time.py measures on a GPU: none found")
    from proxytransformation_amd import QuerySelect, query_select as qs
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    torch.manual_seed(0)
    feats = [torch.from_numpy(rng.standard_normal((n, C)).astype(np.float32)).to(dev) for n in ROWS]
    xyz = [torch.from_numpy((rng.integers(-500, 500, (n, 3)) * 0.01).astype(np.float32)).to(dev) for n in ROWS]
    text = torch.from_numpy(rng.standard_normal((len(ROWS), T, C)).astype(np.float32)).to(dev)
    mask = torch.zeros((len(ROWS), T), dtype=torch.bool)
    for b in range(len(ROWS)):
        mask[b, :int(rng.integers(10, T + 1))] = True
    mask = mask.to(dev)
    m = QuerySelect(embed_dims=C, num_queries=QUERIES)
    with torch.no_grad():
        for lin in m.linears():
            lin.weight.normal_(0.0, (2.0 / C) ** 0.5)
            lin.bias.normal_(0.0, 0.5)
        m.linears()[-1].bias[3:6] -= 3.9
    m = m.to(dev).eval()
    mt = QuerySelect(embed_dims=C, num_queries=QUERIES, differentiable=True).to(dev)
    mt.load_state_dict(m.state_dict())
    reg, cls_bias = m.reg_branch, m.cls_branch.bias
    Lmax, K = max(ROWS), min(QUERIES, min(ROWS))
    G1 = torch.randn((len(ROWS), Lmax, C), device=dev)
    G2 = torch.randn((len(ROWS), K, C), device=dev)
    leaves = [f.clone().requires_grad_() for f in feats]

    def hip_eval():
        with torch.no_grad():
            return m(feats, None, xyz, text, mask)[0]

    def torch_eval():
        with torch.no_grad():
            return torch_stage(feats, xyz, text, mask, cls_bias, reg, QUERIES)[0]

    def hip_train():
        dec = mt(leaves, None, xyz, text, mask)[0]
        return torch.autograd.grad([dec["query"], dec["feats"]], leaves, [G2, G1])

    def torch_train():
        dec = torch_stage(leaves, xyz, text, mask, cls_bias, reg, QUERIES)[0]
        return torch.autograd.grad([dec["query"], dec["feats"]], leaves, [G2, G1])

    lines = [f"QuerySelect(embed_dims={C}, num_queries={QUERIES}) behind MinkNeck; {torch.cuda.get_device_name(0)}; {len(ROWS)} scenes of "
             f"{list(ROWS)} rows (Lmax {Lmax}, {sum(ROWS)} rows in all), T = {T} text tokens, K = {K}",
             f"whole calls through Python, HIP events, median of {args.blocks} blocks of {args.reps} calls after a warm-up block, sides alternating"]
    med, t, last = alternate({"hip": hip_eval, "torch": torch_eval}, args.blocks, args.reps)
    keep = {}
    with torch.no_grad():
        m(feats, None, xyz, text, mask, keep_out=keep)
        t_index = torch_stage(feats, xyz, text, mask, cls_bias, reg, QUERIES)[1]
    same = int((keep["index"] == t_index).sum())
    h, r = last["hip"], last["torch"]
    err = {k: float((h[k] - r[k]).abs().max() / r[k].abs().max()) for k in ("query", "query_coords", "pred_bboxes")} if same == t_index.numel() else {}
    lines.append(f"  eval forward   hip {med['hip']:8.1f} us {spread(t['hip'])}   torch {med['torch']:8.1f} us {spread(t['torch'])}   torch / hip "
                 f"{med['torch'] / med['hip']:5.2f}" + ("   SLOWER than the torch composition" if med["hip"] > med["torch"] else ""))
    lines.append(f"    indices equal to torch.topk's at {same} of {t_index.numel()} places; max |hip - torch| / max |torch|: "
                 + (", ".join(f"{k} {v:.1e}" for k, v in err.items()) if err else "not compared (the selections differ)"))
    med, t, last = alternate({"hip": hip_train, "torch": torch_train}, args.blocks, args.reps)
    gerr = max(float((a - b).abs().max() / b.abs().max()) for a, b in zip(last["hip"], last["torch"])) if same == t_index.numel() else float("nan")
    lines.append(f"  training step  hip {med['hip']:8.1f} us {spread(t['hip'])}   torch {med['torch']:8.1f} us {spread(t['torch'])}   torch / hip "
                 f"{med['torch'] / med['hip']:5.2f}" + ("   SLOWER than the torch composition" if med["hip"] > med["torch"] else ""))
    lines.append(f"    (forward + backward of a gradient on query and feats); max |dfeats hip - torch| / max |torch| {gerr:.1e}")
    # the HIP stage's calls one by one, each one launch, on the chain's own operands
    with torch.no_grad():
        pf, pc, pad, attn = qs.pack(feats, xyz, mask)
        score = qs.score(pf, ROWS, text, mask, cls_bias, True)
        index, inv = qs.topk_sorted(score, ROWS, K, return_inverse=True)
        lins = m.linears()
        h1 = qs.linear(pf, lins[0].weight, lins[0].bias, index)
        h2 = qs.linear(h1, lins[1].weight, lins[1].bias)
        parts = [("pack (k_qs_pack)", lambda: qs.pack(feats, xyz, mask)),
                 ("score (k_qs_gemm<score>)", lambda: qs.score(pf, ROWS, text, mask, cls_bias, True)),
                 ("top-k (k_qs_topk)", lambda: qs.topk_sorted(score, ROWS, K, return_inverse=True)),
                 ("linear 0, gathered (k_qs_gemm<linear>)", lambda: qs.linear(pf, lins[0].weight, lins[0].bias, index)),
                 ("linear 1 (k_qs_gemm<linear>)", lambda: qs.linear(h1, lins[1].weight, lins[1].bias)),
                 ("decode (k_head_boxes<gather>)", lambda: qs.decode(h2, lins[2].weight, lins[2].bias, pf, pc, index)),
                 ("backward (k_qs_bwd)", lambda: qs.select_bwd(G1, G2, inv, ROWS, K, C))]
        lines.append(f"per call of the HIP stage (one launch each, through its Python wrapper), median of {args.blocks} blocks of {args.reps}:")
        total = 0.0
        for name, fn in parts:
            block_us(fn, args.reps)
            us = sorted(block_us(fn, args.reps)[0] for _ in range(args.blocks))
            total += us[len(us) // 2] if not name.startswith("backward") else 0.0
            lines.append(f"  {name:40s} {us[len(us) // 2]:8.1f} us {spread(us)}")
        lines.append(f"  {'sum of the forward calls':40s} {total:8.1f} us")
    text_out = "\n".join(lines) + "\n"
    print(text_out, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text_out)


if __name__ == "__main__":
    main()
