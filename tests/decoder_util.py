"""What the decoder's test modules (and tools/decoder_time.py) share: the entry points, the layer configuration, a module with random
weights and non-trivial BatchNorm statistics, the operands of a call, the torch restatement of the stage with mmcv's wrapper rules, and
the end-to-end case behind ``QuerySelect``.  A plain module: no tests, no marks."""
import functools

import numpy as np
import torch
from torch import nn

from proxytransformation_amd import GroundingDecoder
from tests import query_select_util as qu

DEC_ENTRY_POINTS = ("ptx_dec_posembed", "ptx_dec_linear", "ptx_dec_attention", "ptx_dec_ln", "ptx_dec_boxes", "ptx_dec_scores")
SMALL = dict(C=64, heads=2, ffn=128, layers=2)
E2E = dict(C=256, heads=8, ffn=2048, layers=6)
# more than one group of hoisted key/value projections (4096 // 2C layers per group): 4 + 1 at C = 512 with a head count per attention
# (self, text, scene), 8 + 1 at C = 256
WIDE = dict(C=512, heads=(8, 16, 8), ffn=64, layers=5)
DEEP = dict(C=256, heads=8, ffn=64, layers=9)
GROUP_ROWS, GROUP_K = (65, 1, 130), 3


def group_operands(C, T, seed):
    """The operands of the hoisted-group cases: rows (65, 1, 130), K = 3, ``T`` text tokens, two tokens of scene 1 masked."""
    tm = np.zeros((len(GROUP_ROWS), T), bool)
    tm[1, [0, T - 1]] = True
    return operands(GROUP_ROWS, GROUP_K, T, C, seed, tm)


def scene_alone(ops, b):
    """Scene ``b`` of ``ops`` as a batch of one with its keys cut to its own length."""
    n = int((~ops["key_padding_mask"][b]).sum())
    assert n >= 1 and not ops["key_padding_mask"][b, :n].any()
    cut = lambda a: np.ascontiguousarray(a[b:b + 1, :n])      # noqa: E731
    out = {k: np.ascontiguousarray(v[b:b + 1]) for k, v in ops.items()}
    out.update(key=cut(ops["key"]), key_padding_mask=cut(ops["key_padding_mask"]), key_coords=cut(ops["key_coords"]))
    return out


def layer_cfg(C, heads, ffn):
    """``heads``: one count for the three attentions, or ``(self, text, scene)``."""
    hs, ht, hc = (heads,) * 3 if isinstance(heads, int) else tuple(heads)
    return dict(self_attn_cfg=dict(embed_dims=C, num_heads=hs, dropout=0.0), cross_attn_text_cfg=dict(embed_dims=C, num_heads=ht),
                cross_attn_cfg=dict(embed_dims=C, num_heads=hc), ffn_cfg=dict(embed_dims=C, feedforward_channels=ffn, ffn_drop=0.0))


def module(C=256, heads=8, ffn=2048, layers=6, seed=21, **kw):
    """``GroundingDecoder`` in eval with N(0, 1 / fan_in) matrices, N(0, 0.1) biases, LayerNorm / BatchNorm weights in [0.5, 1.5] and
    running statistics off their initial values."""
    g = torch.Generator().manual_seed(seed)
    m = GroundingDecoder(layers, layer_cfg(C, heads, ffn), **kw)
    with torch.no_grad():
        for name, p in list(m.named_parameters()) + list(m.named_buffers()):
            if not p.is_floating_point():
                continue
            leaf = name.rsplit(".", 1)[-1]
            if p.dim() >= 2:
                fan_in = p[0].numel()
                p.copy_(torch.randn(p.shape, generator=g) / fan_in ** 0.5)
            elif leaf == "running_var" or (leaf == "weight" and p.dim() == 1):
                p.copy_(torch.rand(p.shape, generator=g) + 0.5)
            else:
                p.copy_(torch.randn(p.shape, generator=g) * 0.1)
    return m.eval()


def reg_branches(C, layers, seed=22):
    """One regression branch per layer (Linear + ReLU twice, a Linear to 9), the log-sizes centred on log 0.02 as in
    ``query_select_util.module``."""
    g = torch.Generator().manual_seed(seed)
    out = nn.ModuleList()
    for _ in range(layers):
        br = nn.Sequential(nn.Linear(C, C), nn.ReLU(), nn.Linear(C, C), nn.ReLU(), nn.Linear(C, 9))
        with torch.no_grad():
            for lin in (br[0], br[2], br[4]):
                lin.weight.copy_(torch.randn(lin.weight.shape, generator=g) * (2.0 / C) ** 0.5)
                lin.bias.copy_(torch.randn(lin.bias.shape, generator=g) * 0.5)
            br[4].bias[3:6] -= 3.9
        out.append(br)
    return out.eval()


def operands(rows, K, T, C, seed, text_mask=None):
    """The decoder's operands as fp32 numpy arrays: ``query (B,K,C)``, ``key (B,Lmax,C)`` with zeros on the padding, the padding mask,
    coordinates, 9-value boxes, ``text (B,T,C)`` and ``text_attention_mask (B,T)`` (True = ignore; default: none)."""
    rng = np.random.default_rng(seed)
    B, Lmax = len(rows), max(rows)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)      # noqa: E731
    pad = np.stack([np.arange(Lmax) >= n for n in rows])
    key = np.where(pad[:, :, None], np.float32(0), f(B, Lmax, C))
    kcoords = np.where(pad[:, :, None], np.float32(0), (rng.integers(-500, 500, (B, Lmax, 3)) * 0.01).astype(np.float32))
    boxes = f(B, K, 9)
    boxes[..., 3:6] = np.abs(boxes[..., 3:6]) + 0.02
    tmask = np.zeros((B, T), bool) if text_mask is None else np.asarray(text_mask, bool)
    return dict(query=f(B, K, C), key=key, key_padding_mask=pad, query_coords=(rng.integers(-500, 500, (B, K, 3)) * 0.01).astype(np.float32),
                key_coords=kcoords, pred_bboxes=boxes, text_feats=f(B, T, C), text_attention_mask=tmask)


def host(m, ops, branches, dtype, **kw):
    return m.forward_host(ops["query"], ops["key"], ops["key_padding_mask"], ops["query_coords"], ops["key_coords"], ops["pred_bboxes"],
                          ops["text_feats"], ops["text_attention_mask"], branches, dtype=dtype, **kw)


def device(m, ops, branches, dev="cuda:0"):
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in ops.items()}
    return m(t["query"], t["key"], t["key"], t["key_padding_mask"], None, None, t["query_coords"], t["key_coords"], t["pred_bboxes"],
             t["text_feats"], t["text_attention_mask"], branches)


# ------------------------------------------------------------------------------------------------------------------ torch restatement
def _twin(new, src, dtype, dev):
    """A fresh torch module with ``src``'s state in ``dtype`` on ``dev``, in eval."""
    new.load_state_dict({k: v.detach().cpu() for k, v in src.state_dict().items()})
    return new.to(dtype).to(dev).eval()


def _mha_twin(wrapper, dtype, dev):
    return _twin(nn.MultiheadAttention(wrapper.embed_dims, wrapper.num_heads, batch_first=True), wrapper.attn, dtype, dev)


def _pos_twin(pe, dtype, dev):
    C, cin = pe.position_embedding_head[0].out_channels, pe.position_embedding_head[0].in_channels
    head = _twin(nn.Sequential(nn.Conv1d(cin, C, 1), nn.BatchNorm1d(C), nn.ReLU(), nn.Conv1d(C, C, 1)), pe.position_embedding_head, dtype, dev)
    return lambda x: head(x.transpose(1, 2).contiguous()).transpose(1, 2).contiguous()


def _wrapped(attn, query, key, value, query_pos, key_pos, mask):
    """mmcv's ``MultiheadAttention.forward`` (batch_first): the ``key_pos`` default, positions on q and k only, identity + output."""
    identity = query
    if key_pos is None and query_pos is not None and query_pos.shape == key.shape:
        key_pos = query_pos
    q = query + query_pos if query_pos is not None else query
    k = key + key_pos if key_pos is not None else key
    return identity + attn(q, k, value, key_padding_mask=mask, need_weights=False)[0]


def torch_twin(m, branches, dtype=torch.float64, dev="cpu"):
    """The stage as a user would assemble it from torch modules, with this module's parameters, built once: a callable
    ``ops (dict of tensors on dev) -> (hidden (NL,B,K,C), boxes (NL,B,K,9))``."""
    C = m.embed_dims
    self_pos, cross_pos = _pos_twin(m.self_posembed, dtype, dev), _pos_twin(m.cross_posembed, dtype, dev)
    norm = _twin(nn.LayerNorm(C), m.norm, dtype, dev)
    layers = []
    for lid, layer in enumerate(m.layers):
        fc1, fc2 = layer.ffn.layers[0][0], layer.ffn.layers[1]
        layers.append(dict(
            attn=[_mha_twin(a, dtype, dev) for a in (layer.self_attn, layer.cross_attn_text, layer.cross_attn)],
            norms=[_twin(nn.LayerNorm(C), src, dtype, dev) for src in layer.norms],
            l1=_twin(nn.Linear(fc1.in_features, fc1.out_features), fc1, dtype, dev),
            l2=_twin(nn.Linear(fc2.in_features, fc2.out_features), fc2, dtype, dev),
            reg=_twin(nn.Sequential(*[nn.Linear(x.in_features, x.out_features) if isinstance(x, nn.Linear) else nn.ReLU()
                                      for x in branches[lid]]), branches[lid], dtype, dev)))

    def run(t):
        query, boxes, hidden, all_boxes = t["query"], t["pred_bboxes"], [], []
        with torch.no_grad():
            for d in layers:
                query_pos = self_pos(boxes)
                key_pos = cross_pos(t["key_coords"])                               # per layer, as the reference computes it
                sa, ta, ca = d["attn"]
                query = d["norms"][0](_wrapped(sa, query, query, query, query_pos, query_pos, None))
                query = d["norms"][1](_wrapped(ta, query, t["text_feats"], t["text_feats"], query_pos, None, t["text_attention_mask"]))
                query = d["norms"][2](_wrapped(ca, query, t["key"], t["key"], query_pos, key_pos, t["key_padding_mask"]))
                query = d["norms"][3](query + d["l2"](torch.relu(d["l1"](query))))
                p = d["reg"](query)
                boxes = torch.cat([p[..., :3] + t["query_coords"], torch.exp(p[..., 3:6]).clamp(min=2e-2), p[..., 6:]], -1)
                hidden.append(norm(query))
                all_boxes.append(boxes)
        return torch.stack(hidden), torch.stack(all_boxes)

    return run


def torch_stage(m, ops, branches, dtype=torch.float64, dev="cpu"):
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in ops.items()}
    t = {k: v.to(dtype) if v.is_floating_point() else v for k, v in t.items()}
    return torch_twin(m, branches, dtype, dev)(t)


# ------------------------------------------------------------------------------------------------------------------ the end-to-end case
def e2e_modules():
    return qu.module(), module(**E2E)


def e2e_host(index=None):
    """The fp32 and float64 host chains of the end-to-end case -- ``QuerySelect.forward_host`` on ``query_select_util.e2e_inputs()`` (on
    ``index``, the device's selection, when given), the decoder's ``forward_host`` behind it and the head scores: ``{dtype: (hidden,
    boxes, scores)}``."""
    key = None if index is None else np.asarray(index).tobytes()
    return _e2e_host(key, None if index is None else tuple(np.asarray(index).shape))


@functools.lru_cache(maxsize=2)
def _e2e_host(index_bytes, shape):
    from proxytransformation_amd import decoder_host
    index = None if index_bytes is None else np.frombuffer(index_bytes, np.int64).reshape(shape)
    feats, xyz, text, mask = qu.e2e_inputs()
    qs, dec = e2e_modules()
    out = {}
    for dt in (np.float32, np.float64):
        d, head = qs.forward_host(feats, None, xyz, text, mask, dt, index=index)
        ops = dict(query=d["query"], key=d["feats"], key_padding_mask=d["feats_attention_mask"], query_coords=d["query_coords"],
                   key_coords=d["feats_coords"], pred_bboxes=d["pred_bboxes"], text_feats=d["text_feats"],
                   text_attention_mask=d["text_attention_mask"])
        hidden, boxes = host(dec, ops, qs, dt)
        bias = qs.cls_branch.bias.detach().numpy().astype(dt) if qs.has_bias else None
        scores = decoder_host.contrastive_scores_host(hidden, head["text_feats"], head["text_token_mask"], bias, qs.scaled, qs.max_text_len)
        assert hidden.dtype == dt and boxes.dtype == dt and scores.dtype == dt
        out[np.dtype(dt).name] = (hidden, boxes, scores)
    return out
