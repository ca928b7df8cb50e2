"""What the decoder-training test modules (and tools/decoder_train_time.py) share: the entry points, the cases of the three new operators
with their operands, their references -- the same composition in plain torch on the CPU under autograd, in float32 (the yardstick of
``sparse_util.hold``) and float64 (the reference), computed once and never changed --, the cases of the assembled decoder with its
train-mode torch twin, and the bounds of the gradients that are zero in exact arithmetic.  A plain module: no tests, no marks."""
import functools
import math

import numpy as np
import torch
from torch import nn

from proxytransformation_amd import decoder_grad_host as gh

ENTRY_POINTS = ("ptx_dec_train_workspace_bytes", "ptx_dec_posembed_stats", "ptx_dec_posembed_hidden", "ptx_dec_posembed_bwd",
                "ptx_dec_boxes_bwd", "ptx_dec_scores_bwd")
BN_EPS, MOMENTUM = 1e-5, 0.1
U = 2.0 ** -24                                             # the unit roundoff of fp32


def f64(a):
    return None if a is None else np.asarray(a, np.float64)


# ------------------------------------------------------------------------------------------------------------------ posembed
# (cin, C, rows, shift, padded): the smallest batch torch accepts; a partial 64-row tile of the forward behind a whole one, all 9 inputs;
# 512 channels (8 column tiles) with 130 rows; the same off the origin -- inputs around 100 with unit spread and, as ``cross_posembed``
# meets them, zero rows behind (the padding ``pack`` writes: the last quarter of the rows)
PE_CASES = [(3, 64, 2, 0.0, False), (9, 64, 65, 0.0, False), (3, 512, 130, 0.0, False), (9, 64, 65, 100.0, True), (3, 512, 130, 100.0, True)]
# Off the origin WITHOUT padding zhat = (z - mean) rstd is the difference of two numbers near 100 |w|, so it carries 100 roundings of
# fp32 whoever forms it, and everything behind it inherits them: the fp32 CPU torch chain itself is about 1e-5 off float64 in ``out``
# and ``dconv2_w`` and 4e-4 in ``dconv1_w`` (100 times the rounding of ``sum dz``, which is zero in exact arithmetic) -- at or above the
# 1e-5 ceiling that ``sparse_util.hold`` puts on its yardstick.  This one case goes by the same ratio, 8 times the fp32 torch chain's
# error, without the ceiling (``hold_ratio``).
PE_UNPADDED = (9, 64, 65, 100.0, False)
# The row-slab reductions beyond their first slab (``tr_plan`` of csrc/dec_train_plan.h: 256-row chunks, at most 1024 slabs of ``per``
# chunks each).  257 rows: S = 2, the second slab holds one row; 513 rows with all nine inputs: S = 3, the last slab one row; 512
# channels (eight tiles) over two slabs off the origin with the padded quarter: the slab means differ by about 100 |w|, so the delta
# term of Chan's merge carries the variance.  The fp32 torch chain is within 2.9e-6 of float64 on all three (the largest: ``dconv1_w`` of
# the shifted case).  (9, 64, 513, 100.0, True) is NOT drawn: its ``dconv1_w`` yardstick sits on ``hold``'s 1e-5 ceiling.
PE_SLAB_CASES = [(3, 64, 257, 0.0, False), (9, 64, 513, 0.0, False), (3, 512, 257, 100.0, True)]
# The smallest n with two chunks per slab: 1025 chunks, per = 2, S = 513.  Every full slab merges two chunks (the ``ci >= 1`` iterations,
# Chan's merge between chunks, ``k_pe_fold``'s ``slab_rows = per * 256``); the last slab holds ONE row, so its second chunk index lies
# behind the end and takes the ``break``.  Shifted and padded for the reason above.  The fp32 torch chain sums 262145 rows in float, which
# puts two of its leaves at or near ``hold``'s ceiling (measured on a CPU: out 6.1e-7, running_mean 7.4e-8, running_var 8.7e-8, dconv1_w
# 6.1e-6, dbn_w 2.5e-6, dbn_b 3.9e-6, dconv2_w 1.2e-6, dconv2_b 1.0e-5; the values may move with the CPU's thread count).  So this one
# case goes by ``hold_ratio`` -- 8 times the fp32 chain's error, no ceiling on the yardstick -- AND the device's error against float64
# may be at most ``PE_CHUNK_CAP = 8e-5``: the most ``hold`` lets through anywhere, 8 times its 1e-5 ceiling.
# ``dconv1_b`` goes by ``conv1_bias_bound`` as everywhere.  The fp32 torch chain is NO yardstick for it at this size: its float row sum
# leaves 0.33 against a bound of 0.148 (|dconv1_w| up to 5.0e4); the device sums rows in double and is held to the bound.
PE_CHUNK_CASE = (3, 64, 262145, 100.0, True)
PE_CHUNK_CAP = 8e-5
PE_GRADS = ("dconv1_w", "dconv1_b", "dbn_w", "dbn_b", "dconv2_w", "dconv2_b")
PE_PARAMS = ("conv1_w", "conv1_b", "bn_w", "bn_b", "conv2_w", "conv2_b")


@functools.lru_cache(maxsize=None)
def pe_case(cin, C, n, shift, padded=False, seed=0):
    """x (1,n,cin) ~ N(shift, 1), the six parameters, running statistics off their initial values, dout ~ N(0, 1).  With two rows
    zhat is +-d / sqrt(d^2 + eps) with d half their distance in z: the gradient of z is of the order eps / d^3 and what is left of a
    cancellation of O(1) terms, so the two rows are drawn 0.1 apart (N(shift, 0.01)), where it is large enough to be measured."""
    rng = np.random.default_rng(cin * 100003 + C * 1009 + n * 7 + int(shift) + 31 * seed)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)      # noqa: E731
    x = f(1, n, cin) * np.float32(0.1 if n == 2 else 1.0) + np.float32(shift)
    if padded:
        x[:, n - n // 4:] = 0.0
    return dict(x=x, conv1_w=f(C, cin, 1) / np.float32(math.sqrt(cin)), conv1_b=f(C) * np.float32(0.1),
                bn_w=rng.uniform(0.5, 1.5, C).astype(np.float32), bn_b=f(C) * np.float32(0.1),
                conv2_w=f(C, C, 1) / np.float32(math.sqrt(C)), conv2_b=f(C) * np.float32(0.1),
                running_mean=f(C) * np.float32(0.1), running_var=rng.uniform(0.5, 1.5, C).astype(np.float32), dout=f(1, n, C))


def pe_cut(c, rows):
    """The case on its first ``rows`` rows alone (the same parameters and running statistics)."""
    return dict(c, x=np.ascontiguousarray(c["x"][:, :rows]), dout=np.ascontiguousarray(c["dout"][:, :rows]))


def pe_reversed(c, rows):
    """The case with the order of its first ``rows`` rows reversed in ``x`` and in ``dout``: in exact arithmetic no statistic and no
    gradient moves, and ``out`` comes back in the reversed order."""
    x, dout = c["x"].copy(), c["dout"].copy()
    x[:, :rows], dout[:, :rows] = c["x"][:, :rows][:, ::-1], c["dout"][:, :rows][:, ::-1]
    return dict(c, x=x, dout=dout)


def pe_module(c, dtype=torch.float32, dev="cpu"):
    """The reference's ``position_embedding_head`` with the case's state, in training mode."""
    C, cin = c["conv1_w"].shape[:2]
    head = nn.Sequential(nn.Conv1d(cin, C, 1), nn.BatchNorm1d(C, eps=BN_EPS, momentum=MOMENTUM), nn.ReLU(), nn.Conv1d(C, C, 1))
    t = lambda k: torch.from_numpy(c[k])      # noqa: E731
    head.load_state_dict({"0.weight": t("conv1_w"), "0.bias": t("conv1_b"), "1.weight": t("bn_w"), "1.bias": t("bn_b"),
                          "1.running_mean": t("running_mean"), "1.running_var": t("running_var"),
                          "1.num_batches_tracked": torch.tensor(5), "3.weight": t("conv2_w"), "3.bias": t("conv2_b")})
    return head.to(dtype).to(dev).train()


def pe_grads_of(head):
    p = dict(head.named_parameters())
    g = lambda k: p[k].grad.detach().cpu().numpy()      # noqa: E731
    return dict(dconv1_w=g("0.weight")[:, :, 0], dconv1_b=g("0.bias"), dbn_w=g("1.weight"), dbn_b=g("1.bias"),
                dconv2_w=g("3.weight")[:, :, 0], dconv2_b=g("3.bias"))


def pe_torch(c, dtype, repeat=1):
    """``repeat`` train-mode calls of the torch module on the CPU in ``dtype``, the backward of the last one under ``dout``: a dict with
    ``out``, the six gradients, the running statistics and ``num_batches_tracked``."""
    head = pe_module(c, dtype)
    x = torch.from_numpy(c["x"]).to(dtype).transpose(1, 2).contiguous()
    for _ in range(repeat):
        out = head(x).transpose(1, 2)
    (out * torch.from_numpy(c["dout"]).to(dtype)).sum().backward()
    res = pe_grads_of(head)
    res.update(out=out.detach().numpy(), running_mean=head[1].running_mean.numpy(), running_var=head[1].running_var.numpy(),
               num_batches_tracked=int(head[1].num_batches_tracked))
    return res


@functools.lru_cache(maxsize=None)
def pe_refs(cin, C, n, shift, padded=False, repeat=1):
    c = pe_case(cin, C, n, shift, padded)
    return pe_torch(c, torch.float32, repeat), pe_torch(c, torch.float64, repeat)


def pe_spec(c, dtype, repeat=1):
    """The numpy specification on the case in ``dtype``: the same dict as ``pe_torch`` (without the counter)."""
    a = {k: np.asarray(v, dtype) for k, v in c.items()}
    out, _, running = gh.posembed_train_host(a["x"], a["conv1_w"], a["conv1_b"], a["bn_w"], a["bn_b"], a["conv2_w"], a["conv2_b"], BN_EPS,
                                             a["running_mean"], a["running_var"], MOMENTUM, repeat)
    res = gh.posembed_train_bwd_host(a["x"], a["conv1_w"], a["conv1_b"], a["bn_w"], a["bn_b"], a["conv2_w"], a["dout"], BN_EPS)
    res.update(out=out, running_mean=running[0], running_var=running[1])
    return res


def hold_ratio(name, got, ref32, ref64):
    """``sparse_util.hold``'s ratio without its ceiling on the yardstick (``PE_UNPADDED``), both errors printed."""
    from tests import sparse_util as su
    e_gpu, e_cpu = su.rel(got, ref64), su.rel(ref32, ref64)
    print(f"decoder_train {name}: gpu {e_gpu:.3e}  fp32-cpu {e_cpu:.3e}  ratio {e_gpu / max(e_cpu, 1e-30):.2f}")
    assert e_gpu <= 8.0 * e_cpu, (name, e_gpu, e_cpu)
    return e_gpu, e_cpu


def hold_ratio_capped(name, got, ref32, ref64, cap=PE_CHUNK_CAP):
    """``hold_ratio`` and, in addition, the device's error against float64 at most ``cap`` (``PE_CHUNK_CASE``)."""
    e_gpu, e_cpu = hold_ratio(name, got, ref32, ref64)
    assert e_gpu <= cap, (name, e_gpu, cap)
    return e_gpu, e_cpu


def conv1_bias_bound(c):
    """``dconv1_b`` is zero in exact arithmetic: a bias in front of batch statistics moves the mean and nothing else.  What an fp32
    evaluation returns is the rounding of ``db1_c = sum_r dz_rc``, ``dz = gamma rstd (dpre - dbeta / n - zhat dgamma / n)``, whose three
    parts cancel over the rows because ``dbeta = sum dpre`` and ``sum zhat = 0``.  The plain bound of that sum, from the float64
    specification's own terms, with u = 2^-24: every term of it is formed with a handful of roundings (the quotients ``dbeta / n``,
    ``dgamma / n``, the product with ``zhat``, two subtractions, the product with ``gamma rstd``; the rounding of ``dbeta`` and
    ``dgamma`` themselves), each relative to the term's parts, and ``zhat`` is ``(z - mean) rstd`` with the mean rounded to fp32, which
    leaves ``sum zhat`` at up to ``n u |mean| rstd`` instead of zero.  So

        |db1_c| <= 8 u |gamma_c rstd_c| sum_r (|dpre_rc| + |dbeta_c| / n + (|zhat_rc| + |mean_c| rstd_c) |dgamma_c| / n)

    per channel, 8 standing for those roundings (each counted once, with room for the order of the sum).  Returns the (C,) bounds."""
    a = {k: f64(v) for k, v in c.items()}
    x2, w1, n, mean, m2, rstd, zhat, pre = gh._pe_parts(a["x"], a["conv1_w"], a["conv1_b"], a["bn_w"], a["bn_b"], BN_EPS)
    C = w1.shape[0]
    dpre = np.where(pre > 0, a["dout"].reshape(-1, C) @ a["conv2_w"].reshape(C, C), 0.0)
    dbeta, dgamma = dpre.sum(0), (dpre * zhat).sum(0)
    terms = np.abs(dpre) + np.abs(dbeta) / n + (np.abs(zhat) + np.abs(mean) * rstd) * np.abs(dgamma) / n
    return 8.0 * U * np.abs(a["bn_w"] * rstd) * terms.sum(0)


# ------------------------------------------------------------------------------------------------------------------ boxes
BOX_CASES = [(64, 1), (64, 17), (512, 17), (64, 130), (512, 130)]      # (C, rows): one row, a 16-row group and one row, 9 groups
LOG_CLAMP = math.log(0.02)
# ``dW = dp^T h`` over several row slabs (``TR_BOX_DW`` with S > 1): two slabs with one row in the second; 512 channels over three
BOX_SLAB_CASES = [(64, 257), (512, 513)]
# ``bias=None`` (the null ``a.bias`` of ``k_dec_boxes_bwd``): nothing moves the log-sizes to the clamp, so ``h`` is scaled by
# ``BOX_NOBIAS_SCALE`` -- p ~ N(0, 16), about a sixth of the log-sizes below log 0.02 = -3.9
BOX_NOBIAS_CASE = (64, 130)
BOX_NOBIAS_SCALE = 4.0


@functools.lru_cache(maxsize=None)
def box_case(C, n, seed=0, has_bias=True):
    """h (1,n,C) ~ N(0, 1), weight N(0, 1 / C), the size biases at log 0.02, so that the log-sizes fall on both sides of the clamp (about
    half each; at least 1e-3 away from it, redrawn otherwise: next to it the gradient jumps), coords, dboxes ~ N(0, 1).  Without a bias
    (``bias`` is None in the case) the same draw with ``h`` scaled by ``BOX_NOBIAS_SCALE``."""
    for attempt in range(50):
        rng = np.random.default_rng(C * 1009 + n * 7 + 13 * seed + 1000003 * attempt)
        f = lambda *s: rng.standard_normal(s).astype(np.float32)      # noqa: E731
        c = dict(h=f(1, n, C), weight=f(9, C) / np.float32(math.sqrt(C)), bias=f(9) * np.float32(0.1), coords=f(1, n, 3), dboxes=f(1, n, 9))
        c["bias"][3:6] += np.float32(LOG_CLAMP)
        if not has_bias:
            c["h"] *= np.float32(BOX_NOBIAS_SCALE)
            c["bias"] = None
        p = f64(c["h"]).reshape(n, C) @ f64(c["weight"]).T + (f64(c["bias"]) if has_bias else 0.0)
        if np.abs(p[:, 3:6] - LOG_CLAMP).min() > 1e-3:
            return c
    raise AssertionError("no draw away from the clamp")


def box_torch(c, dtype, has_bias=True):
    """The box head in plain torch under autograd; ``has_bias=False``: no bias is added and no ``dbias`` returned."""
    names = ("h", "weight", "bias") if has_bias else ("h", "weight")
    t = {k: torch.from_numpy(c[k]).to(dtype) for k in names + ("coords", "dboxes")}
    for k in names:
        t[k].requires_grad_()
    p = t["h"] @ t["weight"].T
    if has_bias:
        p = p + t["bias"]
    out = torch.cat([p[..., :3] + t["coords"], torch.exp(p[..., 3:6]).clamp(min=2e-2), p[..., 6:]], -1)
    (out * t["dboxes"]).sum().backward()
    res = dict(out=out.detach().numpy(), dh=t["h"].grad.numpy(), dweight=t["weight"].grad.numpy())
    if has_bias:
        res["dbias"] = t["bias"].grad.numpy()
    return res


@functools.lru_cache(maxsize=None)
def box_refs(C, n, has_bias=True):
    c = box_case(C, n, has_bias=has_bias)
    return box_torch(c, torch.float32, has_bias), box_torch(c, torch.float64, has_bias)


# ------------------------------------------------------------------------------------------------------------------ scores
# (NL, B, K, T, M): one of everything (pooled); two layers and scenes, a row tile and one row, T < M off the 4-grid; a full token tile
# and a partial one with three queries
SCORE_CASES = [(1, 1, 1, 1, 1), (2, 2, 65, 5, 70), (1, 3, 3, 77, 256)]
SCORE_C = 64
# (NL, B, K, T, M, C) beyond one channel tile: four tiles (``col0 > 0`` in both launches); exact K and T tiles with T = M; the limits
# of K and T the entry point admits; ``R = NL K`` crossing layers inside a 64-row tile of the reduction at the widest C
SCORE_WIDE_CASES = [(2, 2, 65, 5, 70, 256), (1, 2, 64, 64, 64, 128), (1, 1, 1024, 256, 256, 64), (3, 2, 130, 65, 256, 512)]


def score_mask(B, T, all_masked_scene=False, seed=0):
    """``(B,T)`` bool, True = a token: about a quarter masked, every scene keeps token 0; ``all_masked_scene``: the last scene keeps none."""
    m = np.random.default_rng(77 + B * 31 + T + seed).random((B, T)) > 0.25
    m[:, 0] = True
    if all_masked_scene:
        m[-1] = False
    return m


def score_case(NL, B, K, T, M, seed=0, all_masked_scene=False, C=SCORE_C):
    rng = np.random.default_rng(NL * 100003 + B * 10007 + K * 101 + T * 7 + M + 17 * seed)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)      # noqa: E731
    return dict(hidden=f(NL, B, K, C), text=f(B, T, C), mask=score_mask(B, T, all_masked_scene, seed), bias=f(1), dscores=f(NL, B, K, M),
                M=M)


def score_torch(c, dtype, scaled=True, has_bias=True):
    """ContrastiveEmbed in plain torch; the loss reads the scores at the unmasked tokens only (``-inf`` elsewhere, as a loss would)."""
    hs, text = (torch.from_numpy(c[k]).to(dtype).requires_grad_() for k in ("hidden", "text"))
    bias = torch.from_numpy(c["bias"]).to(dtype).requires_grad_()
    s = hs @ text.transpose(1, 2)[None]
    if scaled:
        s = s / math.sqrt(hs.shape[-1])
    if has_bias:
        s = s + bias
    T = text.shape[1]
    keep = torch.from_numpy(c["mask"])[None, :, None, :].expand(s.shape)
    g = torch.from_numpy(np.nan_to_num(c["dscores"][..., :T])).to(dtype)
    (torch.where(keep, s, torch.zeros_like(s)) * g).sum().backward()
    res = dict(dhidden=hs.grad.numpy(), dtext=text.grad.numpy())
    if has_bias:
        res["dbias"] = bias.grad.numpy()
    return res


def score_spec(c, dtype, scaled=True, has_bias=True):
    return gh.scores_bwd_host(np.asarray(c["hidden"], dtype), np.asarray(c["text"], dtype), c["mask"], np.asarray(c["dscores"], dtype),
                              has_bias, scaled)


# ------------------------------------------------------------------------------------------------------------------ the assembled decoder
ZERO_LEAVES = ("self_posembed.position_embedding_head.0.bias", "cross_posembed.position_embedding_head.0.bias",
               "cross_posembed.position_embedding_head.3.bias")
PE = ".position_embedding_head."


def _train_copy(new, src, dtype, dev="cpu"):
    new.load_state_dict({k: v.detach().cpu() for k, v in src.state_dict().items()})
    return new.to(dtype).to(dev).train()


def train_twin(m, branches, dtype, dev="cpu"):
    """The stage as a user would assemble it from torch modules in ``.train()``, in ``dtype`` on ``dev``, with ``m``'s state, built
    once: the reference's chain (``cross_posembed`` called per layer, the boxes detached between layers, mmcv's wrapper rules).
    Returns ``(run, named, heads)``: ``run(t) -> (out, self_pe, key_pos_all)`` on a dict of tensors; ``named``: the twin's parameters
    under the decoder's names (``reg.{layer}.{name}`` for the regression branches); ``heads``: the two position embeddings."""
    from tests import decoder_util as du
    C = m.embed_dims
    named, heads = {}, {}

    def keep(prefix, mod):
        for n, p in mod.named_parameters():
            named[prefix + n] = p
        return mod

    for name in ("self_posembed", "cross_posembed"):
        src = getattr(m, name).position_embedding_head
        cin = src[0].in_channels
        heads[name] = keep(name + PE, _train_copy(nn.Sequential(nn.Conv1d(cin, C, 1), nn.BatchNorm1d(C), nn.ReLU(), nn.Conv1d(C, C, 1)), src,
                                                  dtype, dev))
    pos = lambda head, x: head(x.transpose(1, 2).contiguous()).transpose(1, 2).contiguous()      # noqa: E731
    norm = keep("norm.", _train_copy(nn.LayerNorm(C), m.norm, dtype, dev))
    layers = []
    for lid, layer in enumerate(m.layers):
        pre = f"layers.{lid}."
        fc1, fc2 = layer.ffn.layers[0][0], layer.ffn.layers[1]
        layers.append(dict(
            attn=[keep(f"{pre}{n}.attn.", _train_copy(nn.MultiheadAttention(C, getattr(layer, n).num_heads, batch_first=True),
                                                      getattr(layer, n).attn, dtype, dev)) for n in ("self_attn", "cross_attn_text", "cross_attn")],
            norms=[keep(f"{pre}norms.{i}.", _train_copy(nn.LayerNorm(C), src, dtype, dev)) for i, src in enumerate(layer.norms)],
            l1=keep(pre + "ffn.layers.0.0.", _train_copy(nn.Linear(fc1.in_features, fc1.out_features), fc1, dtype, dev)),
            l2=keep(pre + "ffn.layers.1.", _train_copy(nn.Linear(fc2.in_features, fc2.out_features), fc2, dtype, dev)),
            reg=keep(f"reg.{lid}.", _train_copy(nn.Sequential(*[nn.Linear(x.in_features, x.out_features) if isinstance(x, nn.Linear) else nn.ReLU()
                                                                 for x in branches[lid]]), branches[lid], dtype, dev))))

    def run(t, capture=False):
        query, boxes, hidden, all_boxes, self_pe, key_pos_all = t["query"], t["pred_bboxes"], [], [], [], []
        for d in layers:
            query_pos = pos(heads["self_posembed"], boxes)
            key_pos = pos(heads["cross_posembed"], t["key_coords"])
            if capture:
                query_pos.retain_grad()
                key_pos.retain_grad()
                self_pe.append((boxes.cpu().numpy().copy(), query_pos))
                key_pos_all.append(key_pos)
            sa, ta, ca = d["attn"]
            query = d["norms"][0](du._wrapped(sa, query, query, query, query_pos, query_pos, None))
            query = d["norms"][1](du._wrapped(ta, query, t["text_feats"], t["text_feats"], query_pos, None, t["text_attention_mask"]))
            query = d["norms"][2](du._wrapped(ca, query, t["key"], t["key"], query_pos, key_pos, t["key_padding_mask"]))
            query = d["norms"][3](query + d["l2"](torch.relu(d["l1"](query))))
            p = d["reg"](query)
            new_boxes = torch.cat([p[..., :3] + t["query_coords"], torch.exp(p[..., 3:6]).clamp(min=2e-2), p[..., 6:]], -1)
            hidden.append(norm(query))
            all_boxes.append(new_boxes)
            boxes = new_boxes.detach().clone()
        out = (torch.stack(hidden), torch.stack(all_boxes)) if m.return_intermediate else (query, new_boxes)
        return out, self_pe, key_pos_all

    return run, named, heads


def train_twin_step(m, branches, ops, G, dtype):
    """One training step of ``train_twin`` on the CPU in ``dtype``: ``loss = sum(out0 * G[0]) + sum(out1 * G[1])``, backward.  Returns
    a dict: ``grads`` under the decoder's parameter names and ``query`` / ``key`` / ``text_feats``; ``buffers`` (the BatchNorms' running
    statistics and counters after the step); ``out``; and what the bounds of the zero leaves need -- ``self_pe``: per layer the boxes
    the embedding saw and the gradient of its result, ``cross_pe``: the key coordinates and every layer's gradient of ``key_pos``."""
    run, named, heads = train_twin(m, branches, dtype)
    t = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in ops.items()}
    t = {k: v.to(dtype) if v.is_floating_point() else v for k, v in t.items()}
    for k in ("query", "key", "text_feats"):
        t[k].requires_grad_()
    out, self_pe, key_pos_all = run(t, capture=True)
    (sum((o * torch.from_numpy(g).to(dtype)).sum() for o, g in zip(out, G))).backward()
    grads = {n: p.grad.numpy() for n, p in named.items() if p.grad is not None}
    grads.update({k: t[k].grad.numpy() for k in ("query", "key", "text_feats")})
    buffers = {name + PE + "1." + k: v.numpy() for name, head in heads.items() for k, v in head[1].named_buffers()}
    zero = lambda a: torch.zeros_like(a) if a.grad is None else a.grad      # noqa: E731
    return dict(grads=grads, buffers=buffers, out=tuple(o.detach().numpy() for o in out),
                self_pe=[(b, zero(qp).numpy()) for b, qp in self_pe],
                cross_pe=(ops["key_coords"], [zero(kp).numpy() for kp in key_pos_all]))


def posembed_bias_bound(m, name, x, dout):
    """``conv1_bias_bound`` for the decoder's position embedding ``name`` on the rows ``x`` under ``dout`` (float64 terms)."""
    head = getattr(m, name).position_embedding_head
    f = lambda p: p.detach().cpu().numpy()      # noqa: E731
    return conv1_bias_bound(dict(x=x, conv1_w=f(head[0].weight), conv1_b=f(head[0].bias), bn_w=f(head[1].weight), bn_b=f(head[1].bias),
                                 conv2_w=f(head[3].weight), dout=dout))


def zero_leaf_bounds(m, twin64, K):
    """The bounds of the three gradients that are zero in exact arithmetic, from the float64 twin's own terms (``twin64``: what
    ``train_twin_step`` returned in float64), per channel.

    The two first-layer biases stand in front of a training BatchNorm: ``conv1_bias_bound`` on what each embedding saw --
    once per layer, under that layer's gradient of the embedding's result, and the layers' bounds add up (the reference calls
    ``cross_posembed`` per layer too; the hoisted launch meets the sum of those gradients, which the sum of the bounds covers).

    ``cross_posembed...3.bias`` is the column sum of the gradient ``g`` of ``key_pos``: a constant added to every key moves no
    softmax, so every column of every layer's ``g`` sums to zero.  The sum itself runs in double; what is left is the rounding of its terms.  Every
    ``g[r, c]`` is an fp32 sum of ``C`` products (the key projection's backward) of values that are themselves fp32 sums over the ``K``
    queries (the attention's ``dK``), each with the roundings of the probabilities in front of it: ``(C + K + 16) u`` relative to the
    term, the term's magnitude standing for the magnitude of its forming sum, and the layers add up:

        |db2_c| <= (C + K + 16) u sum_r |g[r, c]| (summed over the layers' shares)."""
    C = m.embed_dims
    self_b = sum(posembed_bias_bound(m, "self_posembed", x, g) for x, g in twin64["self_pe"])
    x, gs = twin64["cross_pe"]
    return {ZERO_LEAVES[0]: self_b, ZERO_LEAVES[1]: sum(posembed_bias_bound(m, "cross_posembed", x, g) for g in gs),
            ZERO_LEAVES[2]: (C + K + 16) * U * sum(np.abs(f64(g)).reshape(-1, C).sum(0) for g in gs)}


@functools.lru_cache(maxsize=None)
def dec_case(name):
    """The cases of the assembled decoder: ``(module kwargs, rows, K, T, return_intermediate, text mask)``.  ``small``: two row tiles
    and one row of queries, a partial key tile; ``T == K``: mmcv's rule hands the text keys ``query_pos``; ``groups``: five layers at
    C = 512 are two hoisted groups (4 + 1); ``last``: ``return_intermediate=False``; ``shifted``: the key coordinates moved by 100;
    ``no-token``: a scene with every text token masked."""
    from tests import decoder_util as du
    return dict(small=(du.SMALL, (70, 33), 65, 5, True), tk=(du.SMALL, (70, 33), 5, 5, True),
                groups=(dict(C=512, heads=(8, 16, 8), ffn=64, layers=5), (65, 1, 130), 3, 5, True),
                last=(du.SMALL, (70, 33), 65, 5, False), shifted=(du.SMALL, (70, 33), 65, 5, True),
                notoken=(du.SMALL, (70, 33), 65, 5, True))[name]


@functools.lru_cache(maxsize=None)
def dec_setup(name):
    """``(module (CPU, train mode), branches, operands, G)`` of a case, built once."""
    from tests import decoder_util as du
    cfg, rows, K, T, inter = dec_case(name)
    m = du.module(**cfg, return_intermediate=inter, differentiable=True).train()
    branches = du.reg_branches(cfg["C"], cfg["layers"]).train()
    tm = np.zeros((len(rows), T), bool)
    tm[0, T - 1] = True
    if name == "notoken":
        tm[-1] = True
    ops = du.operands(rows, K, T, cfg["C"], 900 + len(name), tm)
    if name == "shifted":
        ops["key_coords"] = np.where(ops["key_padding_mask"][:, :, None], np.float32(0), ops["key_coords"] + np.float32(100))
    rng = np.random.default_rng(7 + len(name))
    NL, B, C = cfg["layers"], len(rows), cfg["C"]
    shape = (NL, B, K) if inter else (B, K)
    G = (rng.standard_normal(shape + (C,)).astype(np.float32), rng.standard_normal(shape + (9,)).astype(np.float32))
    return m, branches, ops, G


@functools.lru_cache(maxsize=None)
def dec_refs(name):
    m, branches, ops, G = dec_setup(name)
    return train_twin_step(m, branches, ops, G, torch.float32), train_twin_step(m, branches, ops, G, torch.float64)


def spec_step(m, branches, ops, G, dtype=np.float64):
    """The same step through the numpy specification of the whole chain (``decoder_grad_host.decoder_train_host``): ``(out, grads)``."""
    lins = [[x for x in br if isinstance(x, nn.Linear)] for br in branches]
    layer = m.layers[0]
    arr = lambda t: t.detach().cpu().numpy()      # noqa: E731
    return gh.decoder_train_host({k: arr(v) for k, v in m.state_dict().items()}, m.num_layers,
                                 (layer.self_attn.num_heads, layer.cross_attn_text.num_heads, layer.cross_attn.num_heads), ops["query"],
                                 ops["key"], ops["key_padding_mask"], ops["query_coords"], ops["key_coords"], ops["pred_bboxes"],
                                 ops["text_feats"], ops["text_attention_mask"], [[arr(x.weight) for x in ls] for ls in lins],
                                 [[arr(x.bias) for x in ls] for ls in lins], G, dtype, m.return_intermediate)
