"""Query selection behind ``MinkNeck``: the detector's ``pre_decoder`` (detectors/sparse_featfusion_grounder_preshape.py:498-580, the same
body in sparse_featfusion_grounder.py:325-407) on the device.  It turns the three lists ``MinkNeck.forward`` returns into the operands of
the transformer decoder (``decoder.py``): pad to a batch, score every row against the text tokens (``ContrastiveEmbed`` and its maximum
over the tokens), take the per-scene top ``num_queries`` rows in sorted order, run the regression branch and decode 9-value boxes on the
selected rows, gather queries and coordinates.

Six calls into ``csrc/query_select.hip`` on the current stream -- ``pack``, ``score``, ``topk_sorted``, ``linear`` (once per hidden layer
of the regression branch), ``decode`` and, in training, ``select_bwd`` -- each restated in numpy by ``query_select_host.py``, which is
their specification.  No device synchronise, no torch op on the data path: ``Lmax``, ``min L`` and every ``L_b`` are tensor sizes.  fp32
throughout; no float atomics and fixed summation orders, so two calls give the same bits.  The regression branch runs AFTER the
selection: its rows are independent, so this is the reference's result on those rows at ``K / sum L`` of the work.

Parity-unpinned against torch: the tie rule of the top-k (the lower row first) and the place of a sign-set NaN
(``query_select_host.py``).

Training (``QuerySelect(..., differentiable=True)``): one autograd node covers ``feats_list -> (feats, query)``;
``dfeats_b[r] = dfeats[b, r] (+ dquery[b, q] where index[b, q] = r)`` in one kernel through the inverse index.  Scores and selection see
detached values, as ``torch.topk(...)[1]`` does; the text, the coordinates and the regression branch get no gradient from this stage
(``pred_bboxes.detach()``).

Out of scope: the head's loss (the decoder layers are ``decoder.py``), ``num_reg=12``, the FCAF coder, a learnable ``log_scale``, double backward, bf16.
There is no CPU path: tensors must be on the GPU and the library must be built."""
from __future__ import annotations

import ctypes
import math
from typing import List, Optional, Sequence

import numpy as np
import torch
from torch import nn

from . import _abi, query_select_host
from ._doors import (MAX_QUERIES, MAX_SCENES, MAX_TEXT, _f32, _f32_grad, _gpu, _index, _int32_array, _mask_bytes, _np, _ptr, _stream, _train,
                     _width)

__all__ = ["QuerySelect", "decode", "linear", "pack", "score", "select_bwd", "topk_sorted"]

def _pointers(tensors: Sequence[torch.Tensor]):
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() if t.numel() else None for t in tensors])


def pack(feats_list: Sequence[torch.Tensor], xyz_list: Sequence[torch.Tensor], text_token_mask: torch.Tensor):
    """``(feats (B,Lmax,C), coords (B,Lmax,3), pad_mask (B,Lmax) bool, text_attention_mask (B,T) bool)``: scene b's rows at ``[b, :L_b]``
    with zeros behind them, ``pad_mask`` True on padding, ``text_attention_mask = ~text_token_mask`` (``query_select_host.pack_host``, bit
    for bit; ``ptx_qs_pack``, one launch)."""
    B = len(feats_list)
    if not 1 <= B <= MAX_SCENES or len(xyz_list) != B:
        raise ValueError(f"pack: 1 to {MAX_SCENES} scenes with one coordinate tensor each, got {B} and {len(xyz_list)}")
    _gpu("pack", *feats_list, *xyz_list)
    dev = feats_list[0].device
    feats_list = [_f32(f, "pack", dev) for f in feats_list]
    xyz_list = [_f32(p, "pack", dev) for p in xyz_list]
    C = _width("pack", feats_list[0].shape[1] if feats_list[0].dim() == 2 else -1)
    rows = [int(f.shape[0]) for f in feats_list]
    for b, (f, p) in enumerate(zip(feats_list, xyz_list)):
        if f.dim() != 2 or f.shape[1] != C or tuple(p.shape) != (rows[b], 3):
            raise ValueError(f"pack: scene {b}: feats ({rows[b]},{C}) and xyz ({rows[b]},3) expected, got {tuple(f.shape)}, {tuple(p.shape)}")
    Lmax = max(rows)
    if Lmax < 1:
        raise ValueError("pack: every scene is empty")
    T = int(text_token_mask.shape[-1])
    mask = _mask_bytes("pack", "text_token_mask", text_token_mask, (B, T))
    if not 1 <= T <= MAX_TEXT:
        raise ValueError(f"pack: 1 to {MAX_TEXT} text tokens, got {T}")
    feats = torch.empty((B, Lmax, C), dtype=torch.float32, device=dev)
    coords = torch.empty((B, Lmax, 3), dtype=torch.float32, device=dev)
    pad = torch.empty((B, Lmax), dtype=torch.bool, device=dev)
    attn = torch.empty((B, T), dtype=torch.bool, device=dev)
    _abi.check(_abi.lib().ptx_qs_pack(_pointers(feats_list), _pointers(xyz_list), _int32_array(rows), B, C, Lmax, mask.data_ptr(), T,
                                      feats.data_ptr(), coords.data_ptr(), pad.data_ptr(), attn.data_ptr(), _stream(dev)), "ptx_qs_pack")
    return feats, coords, pad, attn


def score(feats: torch.Tensor, rows: Sequence[int], text_feats: torch.Tensor, text_token_mask: torch.Tensor,
          bias: Optional[torch.Tensor] = None, scaled: bool = True) -> torch.Tensor:
    """``(B,Lmax) fp32``: ``ContrastiveEmbed`` and its maximum over the tokens on the padded ``feats (B,Lmax,C)`` --
    ``max_t (feats[b,r] . text[b,t]) (/ sqrtf(C)) (+ bias)`` over the unmasked tokens, ``-inf`` on the rows behind ``rows[b]`` and in a
    scene without a token, NaN where an unmasked product is NaN (``query_select_host.score_host``; ``ptx_qs_score``, one launch; the
    ``(B,L,T)`` tensor is never materialised)."""
    _gpu("score", feats, text_feats)
    dev = feats.device
    feats, text = _f32(feats, "score", dev), _f32(text_feats, "score", dev)
    if feats.dim() != 3 or text.dim() != 3 or text.shape[0] != feats.shape[0] or text.shape[2] != feats.shape[2]:
        raise ValueError(f"score: feats (B,Lmax,C) and text_feats (B,T,C) expected, got {tuple(feats.shape)}, {tuple(text.shape)}")
    B, Lmax, C = (int(v) for v in feats.shape)
    _width("score", C)
    T = int(text.shape[1])
    if not 1 <= T <= MAX_TEXT or not 1 <= B <= MAX_SCENES or len(rows) != B:
        raise ValueError(f"score: 1 to {MAX_TEXT} text tokens and 1 to {MAX_SCENES} scenes with one row count each, got T={T}, B={B}, "
                         f"{len(rows)} row counts")
    mask = _mask_bytes("score", "text_token_mask", text_token_mask, (B, T))
    bias = _f32(bias, "score", dev)
    out = torch.empty((B, Lmax), dtype=torch.float32, device=dev)
    _abi.check(_abi.lib().ptx_qs_score(feats.data_ptr(), _int32_array(rows), B, Lmax, C, text.data_ptr(), mask.data_ptr(), T, int(bool(scaled)),
                                       _ptr(bias), out.data_ptr(), _stream(dev)), "ptx_qs_score")
    return out


def topk_sorted(scores: torch.Tensor, rows: Sequence[int], k: int, return_inverse: bool = False):
    """``index (B,k) int64`` = ``torch.topk(scores, k, dim=1, sorted=True)[1]`` over the rows ``0 .. rows[b] - 1`` of every scene, in
    descending ``neck_host.topk_key`` with the lower row first among equal keys (``query_select_host.topk_sorted_host``, bit for bit;
    ``ptx_qs_topk``, one launch).  ``1 <= k <= 1024`` and ``k <= rows[b]``.  ``return_inverse``: also ``inv (B,Lmax) int32``, the place
    of every selected row, ``-1`` elsewhere."""
    _gpu("topk_sorted", scores)
    dev = scores.device
    scores = _f32(scores, "topk_sorted", dev)
    if scores.dim() != 2 or len(rows) != scores.shape[0] or not 1 <= scores.shape[0] <= MAX_SCENES:
        raise ValueError(f"topk_sorted: scores (B,Lmax) of 1 to {MAX_SCENES} scenes with one row count each, got {tuple(scores.shape)}, {len(rows)}")
    B, Lmax, k = int(scores.shape[0]), int(scores.shape[1]), int(k)
    if not 1 <= k <= MAX_QUERIES or k > min(int(r) for r in rows):
        raise ValueError(f"topk_sorted: k={k} must be 1 to {MAX_QUERIES} and at most the smallest scene's {min(int(r) for r in rows)} rows")
    index = torch.empty((B, k), dtype=torch.int64, device=dev)
    inv = torch.empty((B, Lmax), dtype=torch.int32, device=dev) if return_inverse else None
    _abi.check(_abi.lib().ptx_qs_topk(scores.data_ptr(), _int32_array(rows), B, Lmax, k, index.data_ptr(), _ptr(inv), _stream(dev)),
               "ptx_qs_topk")
    return (index, inv) if return_inverse else index


def linear(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], index: Optional[torch.Tensor] = None, relu: bool = True):
    """``(B,K,Cout) fp32 = act(rows @ weight.T + bias)``: with ``index (B,K) int64`` the rows are ``x[b, index[b,q]]`` of ``x (B,Lmax,Cin)``
    -- the gather is fused -- else ``x (B,K,Cin)`` itself.  ``weight (Cout,Cin)`` as ``nn.Linear`` holds it; the ReLU keeps a NaN
    (``ptx_qs_linear``, one launch on the exact-fp32 matrix instruction)."""
    _gpu("linear", x)
    dev = x.device
    x, weight, bias = _f32(x, "linear", dev), _f32(weight, "linear", dev), _f32(bias, "linear", dev)
    if x.dim() != 3 or weight.dim() != 2 or weight.shape[1] != x.shape[2]:
        raise ValueError(f"linear: x (B,L,Cin) and weight (Cout,Cin) expected, got {tuple(x.shape)}, {tuple(weight.shape)}")
    B, L, cin = (int(v) for v in x.shape)
    cout = _width("linear", weight.shape[0])
    _width("linear", cin)
    K = L if index is None else _index("linear", index, B)
    out = torch.empty((B, K, cout), dtype=torch.float32, device=dev)
    _abi.check(_abi.lib().ptx_qs_linear(x.data_ptr(), B * L, _ptr(index), B, K, L, weight.data_ptr(), _ptr(bias), cin, cout, int(bool(relu)),
                                        out.data_ptr(), _stream(dev)), "ptx_qs_linear")
    return out


def decode(h: Optional[torch.Tensor], weight: torch.Tensor, bias: Optional[torch.Tensor], feats: torch.Tensor, coords: torch.Tensor,
           index: torch.Tensor):
    """``(query (B,K,C), query_coords (B,K,3), pred_bboxes (B,K,9))``: the gathered rows ``feats[b, index]`` / ``coords[b, index]`` bit
    for bit, and the last Linear ``weight (9,C)`` of the regression branch on ``h (B,K,C)`` (``None``: on the gathered rows) decoded by
    the baseline coder -- ``center = p[0:3] + coords``, ``size = max(expf(p[3:6]), 0.02)`` with a NaN kept, ``euler = p[6:9]``
    (``query_select_host.boxes_host``; ``ptx_qs_decode``, one launch)."""
    _gpu("decode", feats, coords, index)
    dev = feats.device
    h, weight, bias = _f32(h, "decode", dev), _f32(weight, "decode", dev), _f32(bias, "decode", dev)
    feats, coords = _f32(feats, "decode", dev), _f32(coords, "decode", dev)
    if feats.dim() != 3:
        raise ValueError(f"decode: feats (B,Lmax,C) expected, got {tuple(feats.shape)}")
    B, Lmax, C = (int(v) for v in feats.shape)
    _width("decode", C)
    K = _index("decode", index, B)
    if tuple(weight.shape) != (9, C) or (bias is not None and bias.numel() != 9) or tuple(coords.shape) != (B, Lmax, 3) or \
            (h is not None and tuple(h.shape) != (B, K, C)):
        raise ValueError(f"decode: weight (9,{C}), bias (9), coords ({B},{Lmax},3) and h ({B},{K},{C}) expected, got {tuple(weight.shape)}, "
                         f"{None if bias is None else tuple(bias.shape)}, {tuple(coords.shape)}, {None if h is None else tuple(h.shape)}")
    query = torch.empty((B, K, C), dtype=torch.float32, device=dev)
    qcoords = torch.empty((B, K, 3), dtype=torch.float32, device=dev)
    boxes = torch.empty((B, K, 9), dtype=torch.float32, device=dev)
    _abi.check(_abi.lib().ptx_qs_decode(_ptr(h), weight.data_ptr(), _ptr(bias), C, feats.data_ptr(), coords.data_ptr(), index.data_ptr(), B, K,
                                        Lmax, query.data_ptr(), qcoords.data_ptr(), boxes.data_ptr(), _stream(dev)), "ptx_qs_decode")
    return query, qcoords, boxes


def select_bwd(dfeats: Optional[torch.Tensor], dquery: Optional[torch.Tensor], inv: torch.Tensor, rows: Sequence[int], K: int,
               C: int) -> List[torch.Tensor]:
    """The per-scene gradients behind ``(feats, query)``: ``d_b[r] = dfeats[b,r] (+ dquery[b,q] where inv[b,r] = q)``, views of one
    buffer (``query_select_host.backward_host``, bit for bit; ``ptx_qs_bwd``, one launch).  Either gradient may be ``None`` (zeros)."""
    dev = inv.device
    dfeats, dquery = _f32_grad(None if dfeats is None else dfeats.detach()), _f32_grad(None if dquery is None else dquery.detach())
    B, Lmax = int(inv.shape[0]), int(inv.shape[1])
    total = sum(int(r) for r in rows)
    flat = torch.empty((total, C), dtype=torch.float32, device=dev)
    _abi.check(_abi.lib().ptx_qs_bwd(_ptr(dfeats), _ptr(dquery), inv.data_ptr(), _int32_array(rows), B, Lmax, int(K), int(C), flat.data_ptr(),
                                     _stream(dev)), "ptx_qs_bwd")
    out, lo = [], 0
    for r in rows:
        out.append(flat[lo:lo + int(r)])
        lo += int(r)
    return out


def _chain(mod: "QuerySelect", feats_list, xyz_list, text_feats, text_token_mask, K: int, want_inv: bool) -> dict:
    """The stage on detached operands: every output, the score, the index and (``want_inv``) the inverse index."""
    feats, coords, pad, attn = pack(feats_list, xyz_list, text_token_mask)
    rows = [int(f.shape[0]) for f in feats_list]
    B, C = len(rows), int(feats.shape[2])
    dev = feats.device
    out = dict(feats=feats, coords=coords, pad=pad, attn=attn, inv=None)
    if K == 0:                                               # an empty scene: nothing to select, nothing launched for it
        out.update(score=None, index=torch.empty((B, 0), dtype=torch.int64, device=dev), query=feats.new_empty((B, 0, C)),
                   qcoords=feats.new_empty((B, 0, 3)), boxes=feats.new_empty((B, 0, 9)))
        return out
    bias = mod.cls_branch.bias if mod.has_bias else None
    out["score"] = score(feats, rows, text_feats, text_token_mask, bias, mod.scaled)
    got = topk_sorted(out["score"], rows, K, return_inverse=want_inv)
    index, out["inv"] = got if want_inv else (got, None)
    layers = mod.linears()
    h = None
    for i, lin in enumerate(layers[:-1]):
        h = linear(feats if i == 0 else h, lin.weight, lin.bias, index if i == 0 else None, relu=True)
    out["query"], out["qcoords"], out["boxes"] = decode(h, layers[-1].weight, layers[-1].bias, feats, coords, index)
    out["index"] = index
    return out


_OUTPUTS = ("feats", "query", "coords", "pad", "attn", "qcoords", "boxes", "score", "index")


class _SelectFn(torch.autograd.Function):
    """``feats_list -> (feats, query)``; everything else the stage returns (``_OUTPUTS``) is not differentiable."""

    @staticmethod
    def forward(ctx, run, K, *feats_list):
        out = run([f.detach() for f in feats_list], True)
        ctx.set_materialize_grads(False)
        ctx.inv, ctx.rows, ctx.K, ctx.C = out["inv"], [int(f.shape[0]) for f in feats_list], K, int(out["feats"].shape[2])
        ctx.mark_non_differentiable(*[out[k] for k in _OUTPUTS[2:] if out[k] is not None])
        return tuple(out[k] for k in _OUTPUTS)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dfeats, dquery, *_rest):
        if ctx.K == 0:
            dquery = None
        if dfeats is None and dquery is None:
            return (None, None) + (None,) * len(ctx.rows)
        inv = ctx.inv
        if inv is None:                                      # K = 0: the padded features alone
            inv = torch.full((len(ctx.rows), max(ctx.rows)), -1, dtype=torch.int32, device=dfeats.device)
        grads = select_bwd(dfeats, dquery, inv, ctx.rows, max(ctx.K, 1), ctx.C)
        return (None, None) + tuple(g if need else None for g, need in zip(grads, ctx.needs_input_grad[2:]))


class _ClsBranch(nn.Module):
    """The place of ``ContrastiveEmbed`` (grounding_head.py:22-99): its only parameter is the bias ``(1,)``, present when ``bias=True``."""

    def __init__(self, bias: bool):
        super().__init__()
        if bias:
            self.bias = nn.Parameter(torch.tensor([-math.log((1 - 0.01) / 0.01)], dtype=torch.float32))


class QuerySelect(nn.Module):
    """``pre_decoder`` with ``bbox_head.cls_branches[decoder.num_layers]`` (``ContrastiveEmbed(max_text_len, log_scale, bias)``) and
    ``bbox_head.reg_branches[decoder.num_layers]`` (``num_reg_fcs`` x (Linear + ReLU) and a Linear to ``num_reg``) of ``GroundingHead``.
    Parameters by the reference's names below the two branches: ``cls_branch.bias (1,)`` (``bias=True`` only), ``reg_branch.{0,2,..}.weight
    / .bias``; ``load_from_head`` copies them out of a reference checkpoint.

    ``forward(feats_list, scores_list, xyz_list, text_feats, text_token_mask, keep_out=None)`` returns ``(decoder_inputs_dict,
    head_inputs_dict)`` with the reference's keys: ``query (B,K,C)``, ``feats (B,Lmax,C)``, ``feats_attention_mask (B,Lmax)`` bool (True on
    padding), ``query_coords (B,K,3)``, ``feats_coords (B,Lmax,3)``, ``pred_bboxes (B,K,9)`` (no grad), ``text_feats`` (passed through),
    ``text_attention_mask (B,T)`` bool; ``head_inputs_dict = dict(text_feats, text_token_mask)``.  ``K = min(num_queries, min_b L_b)``;
    ``K = 0`` (an empty scene) returns correctly shaped empties and launches nothing for the selection.  ``scores_list`` is accepted and
    unused, as in the reference.  ``keep_out``: a dict that receives ``score (B,Lmax) fp32`` and ``index (B,K) int64``.

    Accepted: ``embed_dims`` a multiple of 64 from 64 to 512, ``1 <= T <= max_text_len <= 256``, ``1 <= B <= 64``,
    ``1 <= num_queries <= 1024``.  ``num_reg=12``, ``box_coder='FCAF'`` and a float ``log_scale`` raise ``NotImplementedError``.
    Inference-only by default: a ``feats_list`` entry that requires grad with grad mode on raises ``NotImplementedError``;
    ``differentiable=True`` records one autograd node ``feats_list -> (feats, query)`` (module docstring)."""

    def __init__(self, embed_dims: int = 256, num_queries: int = 256, num_reg: int = 9, num_reg_fcs: int = 2, log_scale="auto",
                 bias: bool = True, max_text_len: int = 256, box_coder: str = "baseline", differentiable: bool = False):
        super().__init__()
        self.differentiable = bool(differentiable)
        self.embed_dims = _width("QuerySelect", embed_dims)
        if isinstance(log_scale, float):
            raise NotImplementedError(f"QuerySelect: a learnable log_scale ({log_scale}) is not implemented; 'auto', 'none' or None")
        if log_scale not in ("auto", "none", None):
            raise ValueError(f'log_scale should be one of "auto", "none", None, but got {log_scale}')
        if box_coder == "FCAF":
            raise NotImplementedError("QuerySelect: box_coder='FCAF' is not implemented; 'baseline'")
        if box_coder != "baseline":
            raise ValueError(f"QuerySelect: box_coder must be 'baseline' or 'FCAF', got {box_coder!r}")
        if int(num_reg) == 12:
            raise NotImplementedError("QuerySelect: num_reg=12 (the 6D rotation) is not implemented; num_reg=9")
        if int(num_reg) != 9:
            raise ValueError(f"QuerySelect: num_reg must be 9 (or 12, not implemented), got {num_reg}")
        if not 1 <= int(num_queries) <= MAX_QUERIES:
            raise ValueError(f"QuerySelect: num_queries must be 1 to {MAX_QUERIES}, got {num_queries}")
        if not 1 <= int(max_text_len) <= MAX_TEXT:
            raise ValueError(f"QuerySelect: max_text_len must be 1 to {MAX_TEXT}, got {max_text_len}")
        if not 0 <= int(num_reg_fcs) <= 8:
            raise ValueError(f"QuerySelect: num_reg_fcs must be 0 to 8, got {num_reg_fcs}")
        self.num_queries, self.num_reg, self.num_reg_fcs = int(num_queries), int(num_reg), int(num_reg_fcs)
        self.log_scale, self.scaled, self.has_bias = log_scale, log_scale == "auto", bool(bias)
        self.max_text_len, self.box_coder = int(max_text_len), box_coder
        self.cls_branch = _ClsBranch(self.has_bias)
        layers: list = []
        for _ in range(self.num_reg_fcs):
            layers += [nn.Linear(self.embed_dims, self.embed_dims), nn.ReLU()]
        layers.append(nn.Linear(self.embed_dims, self.num_reg))
        self.reg_branch = nn.Sequential(*layers)

    def linears(self) -> List[nn.Linear]:
        return [m for m in self.reg_branch if isinstance(m, nn.Linear)]

    def init_weights(self) -> None:
        """``GroundingHead.init_weights`` (grounding_head.py:220-224) for this branch: the last Linear's weight and bias are zero (the
        ``-2.0`` of the reference goes to ``reg_branches[0]`` only, which is not this one)."""
        with torch.no_grad():
            nn.init.constant_(self.reg_branch[-1].weight, 0.0)
            nn.init.constant_(self.reg_branch[-1].bias, 0.0)

    def load_from_head(self, state_dict: dict, layer: int, prefix: str = "bbox_head.") -> None:
        """Copies ``{prefix}cls_branches.{layer}.*`` and ``{prefix}reg_branches.{layer}.*`` of a reference checkpoint; ``layer`` is
        ``decoder.num_layers`` (6 for the shipped configuration)."""
        own = {}
        for name in self.state_dict():
            branch, rest = name.split(".", 1)
            key = f"{prefix}{branch.replace('_branch', '_branches')}.{int(layer)}.{rest}"
            if key not in state_dict:
                raise KeyError(f"QuerySelect.load_from_head: {key} is missing from the state dict")
            own[name] = state_dict[key]
        self.load_state_dict(own, strict=True)

    def _check(self, feats_list, xyz_list, text_feats, text_token_mask):
        B = len(feats_list)
        if not 1 <= B <= MAX_SCENES or len(xyz_list) != B:
            raise ValueError(f"QuerySelect: 1 to {MAX_SCENES} scenes with one coordinate tensor each, got {B} and {len(xyz_list)}")
        tensors = list(feats_list) + list(xyz_list) + [text_feats, text_token_mask]
        if not all(isinstance(t, torch.Tensor) for t in tensors):
            raise TypeError("QuerySelect: feats_list, xyz_list, text_feats and text_token_mask must hold tensors")
        for b, f in enumerate(feats_list):
            if f.dim() != 2 or f.shape[1] != self.embed_dims:
                raise ValueError(f"QuerySelect: scene {b}: feats (L,{self.embed_dims}) expected, got {tuple(f.shape)}")
        if text_feats.dim() != 3 or text_feats.shape[0] != B or text_feats.shape[2] != self.embed_dims:
            raise ValueError(f"QuerySelect: text_feats ({B},T,{self.embed_dims}) expected, got {tuple(text_feats.shape)}")
        T = int(text_feats.shape[1])
        if not 1 <= T <= self.max_text_len:
            raise ValueError(f"QuerySelect: 1 to max_text_len={self.max_text_len} text tokens, got {T}")
        if tuple(text_token_mask.shape) != (B, T):
            raise ValueError(f"QuerySelect: text_token_mask ({B},{T}) expected, got {tuple(text_token_mask.shape)}")
        _gpu("QuerySelect", *tensors)

    def forward(self, feats_list, scores_list, xyz_list, text_feats, text_token_mask, keep_out: Optional[dict] = None):
        train = _train("QuerySelect", self.differentiable, *[f for f in feats_list if isinstance(f, torch.Tensor)])
        self._check(feats_list, xyz_list, text_feats, text_token_mask)
        rows = [int(f.shape[0]) for f in feats_list]
        K = min(self.num_queries, min(rows))
        if max(rows) == 0:                                   # nothing at all: the shapes, no launch
            dev, B, C, T = text_feats.device, len(rows), self.embed_dims, int(text_feats.shape[1])
            new = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device=dev)          # noqa: E731
            if keep_out is not None:
                keep_out.update(score=new(B, 0), index=new(B, 0, dt=torch.int64))
            dec = dict(query=new(B, 0, C), feats=new(B, 0, C), feats_attention_mask=new(B, 0, dt=torch.bool), query_coords=new(B, 0, 3),
                       feats_coords=new(B, 0, 3), pred_bboxes=new(B, 0, 9), text_feats=text_feats,
                       text_attention_mask=~text_token_mask.to(torch.bool))
            return dec, dict(text_feats=text_feats, text_token_mask=text_token_mask)

        def run(detached, want_inv):
            return _chain(self, detached, xyz_list, text_feats, text_token_mask, K, want_inv)

        if train:
            out = dict(zip(_OUTPUTS, _SelectFn.apply(run, K, *[_f32_grad(f) for f in feats_list])))
        else:
            with torch.no_grad():
                out = run([f.detach() for f in feats_list], False)
        feats, query = out["feats"], out["query"]
        if keep_out is not None:
            keep_out.update(score=out["score"] if out["score"] is not None else torch.full_like(out["pad"], -math.inf, dtype=torch.float32),
                            index=out["index"])
        dec = dict(query=query, feats=feats, feats_attention_mask=out["pad"], query_coords=out["qcoords"], feats_coords=out["coords"],
                   pred_bboxes=out["boxes"], text_feats=text_feats, text_attention_mask=out["attn"])
        return dec, dict(text_feats=text_feats, text_token_mask=text_token_mask)

    def forward_host(self, feats_list, scores_list, xyz_list, text_feats, text_token_mask, dtype=np.float64, index=None,
                     keep_out: Optional[dict] = None):
        """The same chain from ``query_select_host.py`` in numpy ``dtype`` with this module's parameters.  ``index (B,K)``: replaces the
        host's own selection (the device's, when a test holds the device's outputs on the device's rows).  ``keep_out`` receives
        ``score`` and the host's OWN ``index``."""
        dt = np.dtype(dtype)
        lins = self.linears()
        return query_select_host.forward_host(
            [_np(f, dt) for f in feats_list], [_np(p, dt) for p in xyz_list], _np(text_feats, dt), _np(text_token_mask, bool),
            [_np(m.weight, dt) for m in lins], [_np(m.bias, dt) for m in lins],
            cls_bias=_np(self.cls_branch.bias, dt) if self.has_bias else None, scaled=self.scaled, num_queries=self.num_queries, dtype=dt,
            index=None if index is None else _np(index, np.int64), keep_out=keep_out)
