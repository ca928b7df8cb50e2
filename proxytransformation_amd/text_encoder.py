"""``ClipTextEncoder``: the text encoder in front of ``text_feat_map`` -- the eval forward of ``transformers.CLIPTextModel`` (the shipped
``t_type='clip-vit-large-patch14-336'``, detectors/sparse_featfusion_grounder_preshape.py:132-136, 661-668, 740-753) from token ids to
``last_hidden_state`` on the device: pre-norm layers, heads of 64, quick-GELU, a causal mask plus the tokenizer's padding mask.

Per forward: ``ptx_txt_embed``; per layer ``ptx_txt_ln_linear`` (LayerNorm1 -> ``[q|k|v]``: the row statistics, then the GEMM that
normalises its operand while it stages it), ``ptx_txt_attention``, ``ptx_txt_linear`` (out_proj + residual), ``ptx_txt_ln_linear``
(LayerNorm2 -> fc1 -> quick-GELU), ``ptx_txt_linear`` (fc2 + residual; beyond 768 input channels in slices that a second launch adds
in ascending order); ``ptx_txt_ln`` (``final_layer_norm``) -- all in
``csrc/text_encoder.hip`` on the current stream, restated in numpy by ``text_encoder_host.py``, which is their specification.  No device
synchronise, no torch op on the data path; fp32 on the exact-fp32 matrix instruction; no float atomics and fixed summation orders: two
calls give the same bits, and a text's rows do not depend on the other texts of the batch.

The reference trains the encoder with ``lr_mult=0.0``: an eval forward under ``no_grad`` is what its training step does to it.  So the
module is inference-only: its parameters do not require grad, the forward runs under ``no_grad`` and the result is detached.

Parity-unpinned: a key that is not admitted is never read (torch multiplies its value by a zero weight); a query without an admitted key
gets zeros (it cannot occur with ``attention_mask[b, 0]`` true); the parameter names are ``CLIPTextModel``'s as the installed
``transformers`` builds them from a config, not checked against a real checkpoint file.

Out of scope: the tokenizer (host code that needs vocabulary files), training the encoder, other ``t_type``s (RoBERTa, T5, open_clip
towers) and ``hidden_act='gelu'``, bf16 weights.  There is no CPU path: the module must be on the GPU and the library must be built."""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch
from torch import nn

from . import _abi, text_encoder_host
from ._doors import MAX_SCENES, MAX_TEXT, PreparedOperands, _np, _ptr, _stream

__all__ = ["ClipTextEncoder"]

MAX_WIDTH, MAX_MLP = 1280, 5120
HEAD_DIM = 64


class _Embeddings(nn.Module):
    def __init__(self, vocab: int, positions: int, C: int):
        super().__init__()
        self.token_embedding = nn.Embedding(vocab, C)
        self.position_embedding = nn.Embedding(positions, C)


class _Attention(nn.Module):
    def __init__(self, C: int):
        super().__init__()
        self.k_proj, self.v_proj, self.q_proj, self.out_proj = nn.Linear(C, C), nn.Linear(C, C), nn.Linear(C, C), nn.Linear(C, C)


class _Mlp(nn.Module):
    def __init__(self, C: int, I: int):
        super().__init__()
        self.fc1, self.fc2 = nn.Linear(C, I), nn.Linear(I, C)


class _Layer(nn.Module):
    def __init__(self, C: int, I: int, eps: float):
        super().__init__()
        self.self_attn = _Attention(C)
        self.layer_norm1 = nn.LayerNorm(C, eps=eps)
        self.mlp = _Mlp(C, I)
        self.layer_norm2 = nn.LayerNorm(C, eps=eps)


class _Encoder(nn.Module):
    def __init__(self, n: int, C: int, I: int, eps: float):
        super().__init__()
        self.layers = nn.ModuleList([_Layer(C, I, eps) for _ in range(n)])


class _TextModel(nn.Module):
    def __init__(self, vocab: int, positions: int, C: int, I: int, n: int, eps: float):
        super().__init__()
        self.embeddings = _Embeddings(vocab, positions, C)
        self.encoder = _Encoder(n, C, I, eps)
        self.final_layer_norm = nn.LayerNorm(C, eps=eps)


class ClipTextEncoder(PreparedOperands, nn.Module):
    """``ClipTextEncoder(vocab_size=49408, hidden_size=768, intermediate_size=3072, num_hidden_layers=12, num_attention_heads=12,
    max_position_embeddings=77, layer_norm_eps=1e-5, hidden_act='quick_gelu')``: ``CLIPTextConfig``'s keywords, ``CLIPTextModel``'s
    parameter names (``text_model.embeddings.token_embedding.weight``, ``text_model.encoder.layers.{i}.self_attn.q_proj.weight``, ...,
    ``text_model.final_layer_norm.bias``).  ``load_state_dict`` also takes them without the ``text_model.`` prefix and ignores an
    ``embeddings.position_ids`` buffer.

    Accepted: ``hidden_size = 64 * num_attention_heads`` up to 1280, ``intermediate_size`` a multiple of 64 up to 5120, 1 to 64 layers,
    up to 256 positions; a call takes 1 to 64 texts of 1 to ``min(256, max_position_embeddings)`` tokens.  Any ``hidden_act`` other than
    ``'quick_gelu'`` raises ``NotImplementedError``.

    The operands the launches take (the concatenated ``[q|k|v]`` weight) are prepared once and rebuilt when a parameter is replaced or
    its ``_version`` changes (``load_state_dict``, in-place updates): ``_doors.PreparedOperands``."""

    def __init__(self, vocab_size: int = 49408, hidden_size: int = 768, intermediate_size: int = 3072, num_hidden_layers: int = 12,
                 num_attention_heads: int = 12, max_position_embeddings: int = 77, layer_norm_eps: float = 1e-5,
                 hidden_act: str = "quick_gelu"):
        super().__init__()
        who = "ClipTextEncoder"
        if hidden_act != "quick_gelu":
            raise NotImplementedError(f"{who}: hidden_act={hidden_act!r} is not implemented; 'quick_gelu' (the shipped CLIP text tower) only")
        C, I, H = int(hidden_size), int(intermediate_size), int(num_attention_heads)
        if H < 1 or C != HEAD_DIM * H or C > MAX_WIDTH:
            raise ValueError(f"{who}: hidden_size must be 64 * num_attention_heads, up to {MAX_WIDTH} (head dimension 64 only), got "
                             f"{hidden_size} with {num_attention_heads} heads")
        if I < 64 or I % 64 or I > MAX_MLP:
            raise ValueError(f"{who}: intermediate_size must be a multiple of 64 up to {MAX_MLP}, got {intermediate_size}")
        if not 1 <= int(num_hidden_layers) <= 64:
            raise ValueError(f"{who}: num_hidden_layers must be 1 to 64, got {num_hidden_layers}")
        if not 1 <= int(max_position_embeddings) <= MAX_TEXT or int(vocab_size) < 1:
            raise ValueError(f"{who}: max_position_embeddings must be 1 to {MAX_TEXT} and vocab_size positive, got "
                             f"{max_position_embeddings}, {vocab_size}")
        if not float(layer_norm_eps) > 0.0:
            raise ValueError(f"{who}: layer_norm_eps must be positive, got {layer_norm_eps}")
        self.vocab_size, self.hidden_size, self.intermediate_size = int(vocab_size), C, I
        self.num_hidden_layers, self.num_attention_heads = int(num_hidden_layers), H
        self.max_position_embeddings, self.layer_norm_eps, self.hidden_act = int(max_position_embeddings), float(layer_norm_eps), hidden_act
        self.text_model = _TextModel(self.vocab_size, self.max_position_embeddings, C, I, self.num_hidden_layers, self.layer_norm_eps)
        for p in self.parameters():
            p.requires_grad_(False)                          # lr_mult=0.0 in the reference: never trained

    # -- checkpoints
    @staticmethod
    def normalise_names(state_dict) -> dict:
        """``state_dict`` under this module's names: the ``text_model.`` prefix added where a release of ``transformers`` leaves it out,
        an ``embeddings.position_ids`` buffer (older releases save one) dropped."""
        out = {}
        for k, v in state_dict.items():
            if k.endswith("embeddings.position_ids"):
                continue
            out[k if k.startswith("text_model.") else "text_model." + k] = v
        return out

    def load_state_dict(self, state_dict, strict: bool = True, **kw):
        return super().load_state_dict(self.normalise_names(state_dict), strict=strict, **kw)

    # -- the operands the launches take (PreparedOperands._prepare caches them)
    def _build_operands(self, dev) -> dict:
        f = lambda t: t.detach().to(dev, torch.float32).contiguous()      # noqa: E731
        tm = self.text_model
        prep = dict(tok=f(tm.embeddings.token_embedding.weight), pos=f(tm.embeddings.position_embedding.weight),
                    fw=f(tm.final_layer_norm.weight), fb=f(tm.final_layer_norm.bias), layers=[])
        for layer in tm.encoder.layers:
            a = layer.self_attn
            prep["layers"].append(dict(
                ln1=(f(layer.layer_norm1.weight), f(layer.layer_norm1.bias)), ln2=(f(layer.layer_norm2.weight), f(layer.layer_norm2.bias)),
                wqkv=torch.cat([f(a.q_proj.weight), f(a.k_proj.weight), f(a.v_proj.weight)]).contiguous(),
                bqkv=torch.cat([f(a.q_proj.bias), f(a.k_proj.bias), f(a.v_proj.bias)]).contiguous(),
                wo=f(a.out_proj.weight), bo=f(a.out_proj.bias), w1=f(layer.mlp.fc1.weight), b1=f(layer.mlp.fc1.bias),
                w2=f(layer.mlp.fc2.weight), b2=f(layer.mlp.fc2.bias)))
        return prep

    # -- the forward
    def _check_ids(self, input_ids, attention_mask):
        who = "ClipTextEncoder"
        if not isinstance(input_ids, torch.Tensor) or input_ids.dim() != 2 or input_ids.is_floating_point() or input_ids.dtype == torch.bool:
            raise ValueError(f"{who}: input_ids must be an integer tensor (B,T), got "
                             f"{getattr(input_ids, 'dtype', type(input_ids).__name__)} {tuple(getattr(input_ids, 'shape', ()))}")
        B, T = int(input_ids.shape[0]), int(input_ids.shape[1])
        limit = min(MAX_TEXT, self.max_position_embeddings)
        if not 1 <= B <= MAX_SCENES or not 1 <= T <= limit:
            raise ValueError(f"{who}: 1 to {MAX_SCENES} texts of 1 to {limit} tokens (the position table), got B={B}, T={T}")
        if attention_mask is not None and (not isinstance(attention_mask, torch.Tensor) or tuple(attention_mask.shape) != (B, T)):
            raise ValueError(f"{who}: attention_mask must be ({B},{T}) or None, got {tuple(getattr(attention_mask, 'shape', ()))}")
        return B, T

    def forward(self, input_ids: torch.Tensor, attention_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``last_hidden_state (B,T,hidden_size) fp32`` of ``input_ids (B,T)`` (integer, on the CPU or the device) under
        ``attention_mask (B,T)`` (nonzero = a token; None: all).  Ids on the CPU are range-checked there (``ValueError``); an id outside
        the vocabulary that arrives on the device gives a NaN row, with no error and no host wait."""
        B, T = self._check_ids(input_ids, attention_mask)
        dev = self.text_model.final_layer_norm.weight.device
        if dev.type != "cuda":
            raise RuntimeError("ClipTextEncoder (HIP) needs the module on the GPU: there is no CPU path")
        if not input_ids.is_cuda:
            if bool(((input_ids < 0) | (input_ids >= self.vocab_size)).any()):
                raise ValueError(f"ClipTextEncoder: input_ids outside [0, {self.vocab_size})")
        elif input_ids.device != dev:
            raise ValueError(f"ClipTextEncoder: input_ids on {input_ids.device}, the module on {dev}")
        with torch.no_grad():
            ids = input_ids.detach().to(dev, torch.int64).contiguous()
            mask = None if attention_mask is None else (attention_mask.detach().to(dev) != 0).contiguous()
            prep = self._prepare(dev)
            C, I, H, eps = self.hidden_size, self.intermediate_size, self.num_attention_heads, self.layer_norm_eps
            n, lib, st = B * T, _abi.lib(), _stream(dev)
            new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)      # noqa: E731
            x, qkv, attn, hid, out, stats = new(B, T, C), new(n, 3 * C), new(n, C), new(n, I), new(B, T, C), new(n, 2)
            nbytes = max(int(lib.ptx_txt_linear_workspace_bytes(n, C, C)), int(lib.ptx_txt_linear_workspace_bytes(n, I, C)))
            ws = torch.empty((nbytes // 4,), dtype=torch.float32, device=dev) if nbytes else None
            _abi.check(lib.ptx_txt_embed(ids.data_ptr(), B, T, prep["tok"].data_ptr(), prep["pos"].data_ptr(), self.vocab_size,
                                         self.max_position_embeddings, C, x.data_ptr(), st), "ptx_txt_embed")
            for L in prep["layers"]:
                _abi.check(lib.ptx_txt_ln_linear(x.data_ptr(), n, L["ln1"][0].data_ptr(), L["ln1"][1].data_ptr(), eps, L["wqkv"].data_ptr(),
                                                 L["bqkv"].data_ptr(), C, 3 * C, 0, qkv.data_ptr(), stats.data_ptr(), st), "ptx_txt_ln_linear")
                _abi.check(lib.ptx_txt_attention(qkv.data_ptr(), _ptr(mask), B, T, H, attn.data_ptr(), st), "ptx_txt_attention")
                _abi.check(lib.ptx_txt_linear(attn.data_ptr(), n, L["wo"].data_ptr(), L["bo"].data_ptr(), C, C, x.data_ptr(), x.data_ptr(),
                                              _ptr(ws), nbytes, st), "ptx_txt_linear")
                _abi.check(lib.ptx_txt_ln_linear(x.data_ptr(), n, L["ln2"][0].data_ptr(), L["ln2"][1].data_ptr(), eps, L["w1"].data_ptr(),
                                                 L["b1"].data_ptr(), C, I, 1, hid.data_ptr(), stats.data_ptr(), st), "ptx_txt_ln_linear")
                _abi.check(lib.ptx_txt_linear(hid.data_ptr(), n, L["w2"].data_ptr(), L["b2"].data_ptr(), I, C, x.data_ptr(), x.data_ptr(),
                                              _ptr(ws), nbytes, st), "ptx_txt_linear")
            _abi.check(lib.ptx_txt_ln(x.data_ptr(), n, C, prep["fw"].data_ptr(), prep["fb"].data_ptr(), eps, out.data_ptr(), st), "ptx_txt_ln")
        return out

    def forward_host(self, input_ids, attention_mask=None, dtype=np.float64) -> np.ndarray:
        """The same chain in numpy ``dtype`` (``text_encoder_host.forward_host``): the specification.  It calls no device code."""
        ids = _np(input_ids)
        if ids.ndim != 2 or ids.dtype.kind not in "iu":
            raise ValueError(f"ClipTextEncoder.forward_host: input_ids must be integers (B,T), got {ids.dtype} {ids.shape}")
        if ids.shape[1] > self.max_position_embeddings:
            raise ValueError(f"ClipTextEncoder.forward_host: T={ids.shape[1]} exceeds the position table ({self.max_position_embeddings})")
        params = {k: _np(v) for k, v in self.state_dict().items()}
        mask = None if attention_mask is None else _np(attention_mask) != 0
        return text_encoder_host.forward_host(params, ids, mask, self.num_attention_heads, self.layer_norm_eps, dtype)
