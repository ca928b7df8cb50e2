"""What the text encoder's test modules (and tools/text_encoder_time.py) share: seeded weights, ids and masks, a plain torch restatement,
the case table and the cached host references.  A plain module: no tests, no marks.

The weights, from ``np.random.default_rng(seed)`` in the order of ``param_shapes``: Linear weights ~ N(0, (3 * 0.02)^2), every bias
(Linear and LayerNorm) ~ N(0, 0.1^2), LayerNorm weights 1 + N(0, 0.1^2), token embeddings ~ N(0, 0.5^2), position embeddings
~ N(0, 0.1^2) -- activations stay O(1) through the layers.  Drawn in float64 and rounded to float32 once, so every consumer (numpy in
either precision, torch, the device) starts from the same fp32 values."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

VOCAB, POSITIONS, EPS = 97, 77, 1e-5

#: (C, H, I, layers, B, T, mask kind): the smallest shapes that reach each edge of csrc/text_encoder.hip
CASES = [
    (128, 2, 128, 1, 1, 1, "none"),        # T = 1
    (128, 2, 320, 2, 3, 20, "tail"),       # 60 rows, under one row tile; I not a multiple of 128
    (128, 2, 320, 2, 4, 20, "hole"),       # 80 rows: a text straddles the row tile
    (128, 2, 128, 1, 2, 64, "none"),       # the attention's key-tile boundary
    (128, 2, 128, 1, 2, 65, "tail"),       # one past it
    (192, 3, 192, 3, 3, 77, "first"),      # three heads
    (64, 1, 2112, 1, 1, 20, "hole"),       # fc2 beyond the decoder's Cin limit (three slices)
    (768, 12, 3072, 2, 6, 77, "tail"),     # the shipped width
    (1280, 20, 5120, 1, 1, 5, "none"),     # the limits
]
#: the three shapes forward_host was first held to CLIPTextModel at
HOST_CASES = [(128, 2, 320, 2, 4, 20), (192, 3, 192, 3, 3, 77), (768, 12, 3072, 2, 6, 77)]
GOLDEN_SHAPE = (128, 2, 128, 2, 3, 20)
MASK_KINDS = ("none", "tail", "first", "hole")
GOLDEN_KINDS = ("tail", "hole")            # what tests/golden/clip_text_tiny.npz holds (two outputs keep it near 120 KB)


def param_shapes(C, I, layers, vocab=VOCAB, positions=POSITIONS):
    """``[(name, shape, kind)]`` under ``CLIPTextModel``'s names; kind: 'w' Linear weight, 'b' bias, 'g' LayerNorm weight, 'tok', 'pos'."""
    out = [("text_model.embeddings.token_embedding.weight", (vocab, C), "tok"),
           ("text_model.embeddings.position_embedding.weight", (positions, C), "pos")]
    for i in range(layers):
        p = f"text_model.encoder.layers.{i}."
        for proj in ("k_proj", "v_proj", "q_proj", "out_proj"):
            out += [(p + f"self_attn.{proj}.weight", (C, C), "w"), (p + f"self_attn.{proj}.bias", (C,), "b")]
        out += [(p + "layer_norm1.weight", (C,), "g"), (p + "layer_norm1.bias", (C,), "b"),
                (p + "mlp.fc1.weight", (I, C), "w"), (p + "mlp.fc1.bias", (I,), "b"),
                (p + "mlp.fc2.weight", (C, I), "w"), (p + "mlp.fc2.bias", (C,), "b"),
                (p + "layer_norm2.weight", (C,), "g"), (p + "layer_norm2.bias", (C,), "b")]
    out += [("text_model.final_layer_norm.weight", (C,), "g"), ("text_model.final_layer_norm.bias", (C,), "b")]
    return out


def make_params(C, I, layers, seed=0, vocab=VOCAB, positions=POSITIONS):
    """The seeded fp32 weights (module docstring) as ``{name: ndarray}``."""
    rng = np.random.default_rng(seed)
    scale = dict(w=0.06, b=0.1, g=0.1, tok=0.5, pos=0.1)
    out = {}
    for name, shape, kind in param_shapes(C, I, layers, vocab, positions):
        a = rng.standard_normal(shape) * scale[kind]
        out[name] = (1.0 + a if kind == "g" else a).astype(np.float32)
    return out


def make_ids(B, T, seed=0, vocab=VOCAB):
    return np.random.default_rng(1000 + seed).integers(0, vocab, size=(B, T), dtype=np.int64)


def make_mask(kind, B, T):
    """``(B,T)`` bool or None.  'tail': text b keeps its first T - (3 b + 1) % T tokens; 'first': token 0 only; 'hole': positions
    T // 3 .. T // 2 - 1 are padding, the rest are tokens."""
    if kind == "none":
        return None
    m = np.zeros((B, T), bool)
    for b in range(B):
        if kind == "tail":
            m[b, :T - (3 * b + 1) % T] = True
        elif kind == "first":
            m[b, 0] = True
        elif kind == "hole":
            m[b] = True
            m[b, T // 3:T // 2] = False
        else:
            raise ValueError(kind)
    return m


def build_encoder(C, H, I, layers, seed=0, vocab=VOCAB, positions=POSITIONS, params=None):
    """A ``ClipTextEncoder`` of that shape with the seeded weights, on the CPU."""
    from proxytransformation_amd import ClipTextEncoder
    enc = ClipTextEncoder(vocab_size=vocab, hidden_size=C, intermediate_size=I, num_hidden_layers=layers, num_attention_heads=H,
                          max_position_embeddings=positions, layer_norm_eps=EPS)
    params = make_params(C, I, layers, seed, vocab, positions) if params is None else params
    enc.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    return enc.eval()


def torch_forward(params, ids, mask, H, eps=EPS):
    """The plain torch composition of the stage (``F.linear``, ``F.layer_norm``, ``F.scaled_dot_product_attention`` under the causal
    and padding mask) on ``params {name: tensor}`` of any dtype and device: what a user would write without this package."""
    P = lambda n: params["text_model." + n]      # noqa: E731
    B, T = ids.shape
    x = P("embeddings.token_embedding.weight")[ids] + P("embeddings.position_embedding.weight")[:T]
    C = x.shape[-1]
    allow = torch.ones((T, T), dtype=torch.bool, device=x.device).tril()[None, None]
    if mask is not None:
        allow = allow & mask.bool()[:, None, None, :]
    i = 0
    while f"text_model.encoder.layers.{i}.layer_norm1.weight" in params:
        L = lambda n, i=i: P(f"encoder.layers.{i}.{n}")      # noqa: E731
        h = F.layer_norm(x, (C,), L("layer_norm1.weight"), L("layer_norm1.bias"), eps)
        q, k, v = (F.linear(h, L(f"self_attn.{p}_proj.weight"), L(f"self_attn.{p}_proj.bias")).view(B, T, H, C // H).transpose(1, 2)
                   for p in "qkv")
        a = F.scaled_dot_product_attention(q, k, v, attn_mask=allow).transpose(1, 2).reshape(B, T, C)
        x = x + F.linear(a, L("self_attn.out_proj.weight"), L("self_attn.out_proj.bias"))
        h = F.layer_norm(x, (C,), L("layer_norm2.weight"), L("layer_norm2.bias"), eps)
        h = F.linear(h, L("mlp.fc1.weight"), L("mlp.fc1.bias"))
        h = h * torch.sigmoid(1.702 * h)
        x = x + F.linear(h, L("mlp.fc2.weight"), L("mlp.fc2.bias"))
        i += 1
    return F.layer_norm(x, (C,), P("final_layer_norm.weight"), P("final_layer_norm.bias"), eps)


def clip_text_model(params, C, H, I, layers, vocab=VOCAB, positions=POSITIONS):
    """``transformers.CLIPTextModel`` in double, built from a config (never from a checkpoint), with ``params`` loaded."""
    from transformers import CLIPTextConfig, CLIPTextModel
    cfg = CLIPTextConfig(vocab_size=vocab, hidden_size=C, intermediate_size=I, num_hidden_layers=layers, num_attention_heads=H,
                         max_position_embeddings=positions, layer_norm_eps=EPS, hidden_act="quick_gelu", projection_dim=C,
                         attention_dropout=0.0, pad_token_id=0, bos_token_id=1, eos_token_id=2)
    model = CLIPTextModel(cfg).double().eval()
    own = model.state_dict()
    prefixed = any(k.startswith("text_model.") for k in own)
    sd = {(k if prefixed else k[len("text_model."):]): torch.from_numpy(v).double() for k, v in params.items()}
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.endswith("position_ids") for k in missing), (missing, unexpected)
    return model


def err(t, f64):
    """max|t - f64| / max|f64| over every row."""
    return float(np.abs(np.asarray(t, np.float64) - f64).max() / np.abs(f64).max())


@functools.lru_cache(maxsize=None)
def reference(case):
    """``dict(params, ids, mask, f64, f32)`` of a case: ``forward_host`` in both precisions, computed once per process and shared --
    callers must leave the arrays as they are."""
    from proxytransformation_amd import text_encoder_host
    C, H, I, layers, B, T, kind = case
    params, ids, mask = make_params(C, I, layers), make_ids(B, T), make_mask(kind, B, T)
    f64 = text_encoder_host.forward_host(params, ids, mask, H, EPS, np.float64)
    f32 = text_encoder_host.forward_host(params, ids, mask, H, EPS, np.float32)
    return dict(params=params, ids=ids, mask=mask, f64=f64, f32=f32)
