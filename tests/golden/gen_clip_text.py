#!/usr/bin/env python3
"""Generate clip_text_tiny.npz and clip_text_state_dict.json from ``transformers.CLIPTextModel``.

Runs ONLY where ``transformers`` is installed.  The model is built from a ``CLIPTextConfig`` (never from a checkpoint) and carries the
seeded weights of ``tests/text_encoder_util.make_params`` at (C, H, I, layers, B, T) = (128, 2, 128, 2, 3, 20), in double.

clip_text_tiny.npz holds data only: ``ids (3,20) int64``; per mask kind of ``text_encoder_util.GOLDEN_KINDS`` the mask ``mask_<kind> (3,20)
uint8`` and ``out_<kind> (3,20,128) float64`` = ``last_hidden_state``.  The weights are not stored: the recipe and
the seed are.  With it the check of ``forward_host`` does not need ``transformers`` where it runs.

clip_text_state_dict.json: ``[[name, shape], ...]`` of ``CLIPTextModel``'s state dict at the shipped shape (``CLIPTextConfig()`` with
``hidden_size=768, intermediate_size=3072, 12 layers, 12 heads, 77 positions, vocab 49408``), names with the ``text_model.`` prefix that
releases before 5 emit; read off the meta device, so no weight is allocated.  A ``position_ids`` buffer is not listed.

Usage:  python tests/golden/gen_clip_text.py
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)

from tests import text_encoder_util as U      # noqa: E402


def tiny():
    C, H, I, layers, B, T = U.GOLDEN_SHAPE
    params = U.make_params(C, I, layers)
    model = U.clip_text_model(params, C, H, I, layers)
    ids = U.make_ids(B, T)
    out = dict(ids=ids)
    for kind in U.GOLDEN_KINDS:
        mask = U.make_mask(kind, B, T)
        with torch.no_grad():
            res = model(input_ids=torch.from_numpy(ids), attention_mask=None if mask is None else torch.from_numpy(mask).long())
        out[f"out_{kind}"] = res.last_hidden_state.numpy().astype(np.float64)
        if mask is not None:
            out[f"mask_{kind}"] = mask.astype(np.uint8)
    path = os.path.join(HERE, "clip_text_tiny.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


def manifest():
    from transformers import CLIPTextConfig, CLIPTextModel
    cfg = CLIPTextConfig(vocab_size=49408, hidden_size=768, intermediate_size=3072, num_hidden_layers=12, num_attention_heads=12,
                         max_position_embeddings=77, hidden_act="quick_gelu")
    with torch.device("meta"):
        model = CLIPTextModel(cfg)
    rows = []
    for k, v in model.state_dict().items():
        if k.endswith("position_ids"):
            continue
        rows.append([k if k.startswith("text_model.") else "text_model." + k, list(v.shape)])
    path = os.path.join(HERE, "clip_text_state_dict.json")
    with open(path, "w") as f:
        f.write("[\n" + ",\n".join(" " + json.dumps(r) for r in rows) + "\n]\n")
    print(path, len(rows), "tensors")


if __name__ == "__main__":
    tiny()
    manifest()
