"""Training through the decoder on the device: ``posembed`` with a training-mode BatchNorm, ``boxes`` and ``contrastive_scores`` of
proxytransformation_amd/decoder.py with ``differentiable=True`` (csrc/decoder_train.hip) against float64 torch autograd of the same
composition, the fp32 torch chain on the CPU as the yardstick (``sparse_util.hold``: the device error against float64 is at most 8 times
the fp32 chain's; tests/test_decoder_train_host.py asserts the yardstick's precondition on every case drawn here and that the numpy
specification is that float64 chain to 1e-10); forward bits; the mask rule of the scores; the refusals.

Two rules are this module's own.  ``dconv1_b`` of the position embedding is zero in exact arithmetic (a bias in front of batch
statistics) and is held to ``decoder_train_util.conv1_bias_bound``.  A log-size within an ulp of the clamp is decided by
``expf(p) >= 0.02f`` on the device and by float64 ``exp`` in the reference, which may disagree: there either branch's value is accepted
and the verdict must agree with the forward's size."""
import math

import numpy as np
import pytest
import torch

from proxytransformation_amd import decoder
from tests import decoder_grad_util as gu
from tests import decoder_train_util as tu
from tests import sparse_util as su

pytestmark = pytest.mark.gpu
DEV = su.DEV
bits_equal = gu.bits_equal


def dev(a, grad=False):
    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t.requires_grad_() if grad and t.is_floating_point() else t


def host(t):
    return t.detach().cpu().numpy()


# ------------------------------------------------------------------------------------------------------------------ posembed
def run_posembed(c, repeat=1):
    head = tu.pe_module(c, dev=DEV)
    out = decoder.posembed(dev(c["x"]), head, differentiable=True, repeat=repeat)
    (out * dev(c["dout"])).sum().backward()
    res = tu.pe_grads_of(head)
    res.update(out=host(out), running_mean=host(head[1].running_mean), running_var=host(head[1].running_var),
               num_batches_tracked=int(head[1].num_batches_tracked))
    return res


@pytest.mark.parametrize("cin,C,n,shift,padded", tu.PE_CASES + [tu.PE_UNPADDED])
def test_posembed_training_forward_statistics_and_gradients(cin, C, n, shift, padded):
    c = tu.pe_case(cin, C, n, shift, padded)
    r32, r64 = tu.pe_refs(cin, C, n, shift, padded)
    got = run_posembed(c)
    assert got["num_batches_tracked"] == r64["num_batches_tracked"] == 6
    name = f"posembed cin={cin} C={C} n={n} shift={shift} padded={padded}"
    for k in ("out", "running_mean", "running_var") + tu.PE_GRADS:
        assert got[k].shape == r64[k].shape and got[k].dtype == np.float32 and got[k].size >= su.MIN_SAMPLE, k
        if k == "dconv1_b":                                  # zero but for rounding (the module's docstring)
            bound = tu.conv1_bias_bound(c)
            print(f"{name} dconv1_b: |gpu| {np.abs(got[k]).max():.3e}  bound {bound.max():.3e}  |dconv1_w| {np.abs(r64['dconv1_w']).max():.3e}")
            assert (np.abs(got[k]) <= bound).all(), (k, float(np.abs(got[k]).max()), float(bound.max()))
        elif (cin, C, n, shift, padded) == tu.PE_UNPADDED:       # decoder_train_util says why
            tu.hold_ratio(f"{name} {k}", got[k], r32[k], r64[k])
        else:
            su.hold(f"{name} {k}", got[k], r32[k], r64[k])


def test_posembed_running_statistics_after_three_calls_in_one():
    """``repeat=3``: the running statistics and the counter as after three calls of the torch module on the same rows."""
    case = tu.PE_CASES[1]
    c = tu.pe_case(*case)
    r32, r64 = tu.pe_refs(*case, repeat=3)
    got = run_posembed(c, repeat=3)
    assert got["num_batches_tracked"] == r64["num_batches_tracked"] == 8
    for k in ("running_mean", "running_var", "out", "dbn_w"):
        su.hold(f"posembed repeat=3 {k}", got[k], r32[k], r64[k])
    once = run_posembed(c)
    assert bits_equal(once["out"], got["out"]) and not bits_equal(once["running_mean"], got["running_mean"])


def test_posembed_forward_is_the_eval_launch_on_the_device_folded_operands():
    """Stage (c) is ``ptx_dec_posembed`` unchanged: the plain call on ``posembed_folded``'s operands gives the training forward's bits, and
    folding moves no running statistics.  Two runs give the same bits, gradients included."""
    c = tu.pe_case(*tu.PE_CASES[2])
    head = tu.pe_module(c, dev=DEV)
    before = host(head[1].running_mean).copy()
    folded = decoder.posembed_folded(dev(c["x"]), head)
    assert bits_equal(host(head[1].running_mean), before) and int(head[1].num_batches_tracked) == 5
    with torch.no_grad():
        plain = decoder.posembed(dev(c["x"]), folded)
    a, b = run_posembed(c), run_posembed(c)
    assert bits_equal(host(plain), a["out"])
    for k in a:
        assert k == "num_batches_tracked" or bits_equal(a[k], b[k]), k


# ------------------------------------------------------------------------------------------------------------------ boxes
def run_boxes(c):
    t = {k: dev(c[k], k in ("h", "weight", "bias")) for k in ("h", "weight", "bias", "coords", "dboxes")}
    out = decoder.boxes(t["h"], t["weight"], t["bias"], t["coords"], differentiable=True)
    (out * t["dboxes"]).sum().backward()
    return out, dict(dh=host(t["h"].grad), dweight=host(t["weight"].grad), dbias=host(t["bias"].grad))


@pytest.mark.parametrize("C,n", tu.BOX_CASES)
def test_boxes_gradients_on_both_sides_of_the_clamp(C, n):
    r32, r64 = tu.box_refs(C, n)
    if n == 1:                                               # 9 + 64 values a call: pooled over fresh draws of the same shape
        for k in ("dh", "dweight", "dbias"):
            seeds = iter(range(100))
            draw = lambda: (tu.box_case(C, n, next(seeds)),)      # noqa: E731
            su.hold_pooled(f"boxes C={C} n={n} {k}", r64[k].size, draw, lambda c: run_boxes(c)[1][k],
                           lambda c: (tu.box_torch(c, torch.float32)[k], tu.box_torch(c, torch.float64)[k]))
        return
    c = tu.box_case(C, n)
    out, got = run_boxes(c)
    with torch.no_grad():
        plain = decoder.boxes(dev(c["h"]), dev(c["weight"]), dev(c["bias"]), dev(c["coords"]))
    assert bits_equal(host(out), host(plain))
    sizes = host(out)[..., 3:6]
    assert (sizes == np.float32(0.02)).any() and (sizes > np.float32(0.02)).any()      # both sides of the clamp
    for k in ("dh", "dweight", "dbias"):
        assert got[k].shape == r64[k].shape and got[k].dtype == np.float32
        rule = su.hold if got[k].size >= su.MIN_SAMPLE else None
        if rule is None:                                     # dbias: 9 values, pooled with two more draws' below
            continue
        su.hold(f"boxes C={C} n={n} {k}", got[k], r32[k], r64[k])
    seeds = iter(range(100))
    su.hold_pooled(f"boxes C={C} n={n} dbias", 9, lambda: (tu.box_case(C, n, next(seeds)),), lambda c: run_boxes(c)[1]["dbias"],
                   lambda c: (tu.box_torch(c, torch.float32)["dbias"], tu.box_torch(c, torch.float64)["dbias"]))


def test_boxes_next_to_the_clamp_nan_and_infinity():
    """One row, ``h = 0``, so ``p = bias``: the size gradient is ``dbias[3]``.  fp32(log 0.02) is within an ulp of the clamp: either
    branch's value, and the verdict of the forward's size where that tells (a size above 0.02 passed).  A NaN log-size gives NaN, +inf
    gives inf, -inf and a log-size clearly below give 0, one clearly above ``d exp(p)``."""
    h, w, coords = torch.zeros(1, 1, 64, device=DEV), torch.zeros(9, 64, device=DEV), torch.zeros(1, 1, 3, device=DEV)
    d = torch.full((1, 1, 9), 2.0, device=DEV)

    def size_grad(val):
        bias = torch.zeros(9, device=DEV)
        bias[3] = val
        bias.requires_grad_()
        out = decoder.boxes(h, w, bias, coords, differentiable=True)
        (out * d).sum().backward()
        g = host(bias.grad)
        assert (np.delete(g, 3) == 2.0).all()
        return float(host(out)[0, 0, 3]), float(g[3])

    size, g = size_grad(float(np.float32(math.log(0.02))))
    passed = 2.0 * 0.02
    assert g == 0.0 or abs(g - passed) <= 1e-6 * passed, g
    assert size == float(np.float32(0.02)) or (size > 0.02 and g != 0.0)
    assert math.isnan(size_grad(float("nan"))[1]) and size_grad(float("inf"))[1] == float("inf")
    assert size_grad(float("-inf"))[1] == 0.0 and size_grad(-4.0)[1] == 0.0
    assert abs(size_grad(1.0)[1] - 2.0 * math.e) <= 1e-6 * 2.0 * math.e


# ------------------------------------------------------------------------------------------------------------------ scores
def run_scores(c, scaled=True, has_bias=True):
    hs, text, bias = dev(c["hidden"], True), dev(c["text"], True), dev(c["bias"], True) if has_bias else None
    out = decoder.contrastive_scores(hs, text, dev(c["mask"]), bias, scaled, c["M"], differentiable=True)
    out.backward(dev(c["dscores"]))
    res = dict(dhidden=host(hs.grad), dtext=host(text.grad))
    if has_bias:
        res["dbias"] = host(bias.grad)
    return out, res


@pytest.mark.parametrize("NL,B,K,T,M", tu.SCORE_CASES)
def test_scores_gradients(NL, B, K, T, M):
    names = ("dhidden", "dtext", "dbias")
    if NL * B * K * T == 1:                                  # one of everything: pooled over fresh draws
        for k in names:
            seeds = iter(range(200))
            su.hold_pooled(f"scores (1,1,1,1,1) {k}", 1 if k == "dbias" else tu.SCORE_C, lambda: (tu.score_case(NL, B, K, T, M, next(seeds)),),
                           lambda c: run_scores(c)[1][k], lambda c: (tu.score_torch(c, torch.float32)[k], tu.score_torch(c, torch.float64)[k]))
        return
    for scaled, has_bias in ((True, True), (False, False)):
        c = tu.score_case(NL, B, K, T, M)
        out, got = run_scores(c, scaled, has_bias)
        with torch.no_grad():
            plain = decoder.contrastive_scores(dev(c["hidden"]), dev(c["text"]), dev(c["mask"]), dev(c["bias"]) if has_bias else None, scaled, M)
        assert bits_equal(host(out), host(plain))
        r32, r64 = tu.score_torch(c, torch.float32, scaled, has_bias), tu.score_torch(c, torch.float64, scaled, has_bias)
        for k in ("dhidden", "dtext"):
            assert got[k].shape == r64[k].shape and got[k].dtype == np.float32
            su.hold(f"scores {NL, B, K, T, M} scaled={scaled} {k}", got[k], r32[k], r64[k])
        assert not got["dtext"][~c["mask"]].view(np.uint32).any()      # bit zero on a masked token
    seeds = iter(range(200))
    su.hold_pooled(f"scores {NL, B, K, T, M} dbias", 1, lambda: (tu.score_case(NL, B, K, T, M, next(seeds)),),
                   lambda c: run_scores(c)[1]["dbias"], lambda c: (tu.score_torch(c, torch.float32)["dbias"], tu.score_torch(c, torch.float64)["dbias"]))


def test_scores_a_nan_under_the_mask_or_behind_T_leaves_no_trace():
    """A scene with every token masked; NaN planted in the incoming gradient under every masked token and in every column from T on:
    ``dhidden``, ``dtext`` and ``dbias`` are finite and bit for bit those of the clean gradient."""
    c = tu.score_case(2, 2, 65, 5, 70, all_masked_scene=True)
    _, clean = run_scores(c)
    d = c["dscores"].copy()
    d[..., 5:] = np.nan
    d[..., :5][np.broadcast_to(~c["mask"][None, :, None, :], d[..., :5].shape)] = np.nan
    _, dirty = run_scores(dict(c, dscores=d))
    r32, r64 = tu.score_torch(c, torch.float32), tu.score_torch(c, torch.float64)
    for k in clean:
        assert np.isfinite(dirty[k]).all() and bits_equal(clean[k], dirty[k]), k
    for k in ("dhidden", "dtext"):
        su.hold(f"scores with a scene without tokens {k}", clean[k], r32[k], r64[k])
    assert not clean["dhidden"][:, -1].view(np.uint32).any() and not clean["dtext"][-1].view(np.uint32).any()


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_operator_refusals_come_before_any_launch():
    c = tu.pe_case(*tu.PE_CASES[0])
    head = tu.pe_module(c, dev=DEV)
    x = dev(c["x"])
    state = {k: host(v).copy() for k, v in head.state_dict().items()}

    def untouched():
        return all(np.array_equal(host(v), state[k]) for k, v in head.state_dict().items())

    with pytest.raises(NotImplementedError, match="training mode"):
        decoder.posembed(x, head)                            # without the keyword: the present refusal
    with pytest.raises(NotImplementedError, match="x requires grad"):
        decoder.posembed(dev(c["x"], True), head, differentiable=True)
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        decoder.posembed(x[:, :1], head, differentiable=True)
    head.eval()
    with pytest.raises(NotImplementedError, match="frozen BatchNorm"):
        decoder.posembed(x, head, differentiable=True)
    assert untouched()
    for p in head.parameters():
        p.requires_grad_(False)
    with torch.no_grad():
        assert bits_equal(host(decoder.posembed(x, head, differentiable=True)), host(decoder.posembed(x, head)))      # eval, frozen: the eval path
    slot = torch.full((1, 4, 9), 7.0, device=DEV)
    hq = torch.zeros(1, 4, 64, device=DEV, requires_grad=True)
    with pytest.raises(ValueError, match="out cannot be given"):
        decoder.boxes(hq, torch.zeros(9, 64, device=DEV), None, torch.zeros(1, 4, 3, device=DEV), out=slot, differentiable=True)
    assert bool((slot == 7.0).all())
    assert not decoder.boxes(hq, torch.zeros(9, 64, device=DEV), None, torch.zeros(1, 4, 3, device=DEV)).requires_grad
    sc = tu.score_case(1, 3, 3, 77, 256)
    assert not decoder.contrastive_scores(dev(sc["hidden"], True), dev(sc["text"]), dev(sc["mask"])).requires_grad


# ------------------------------------------------------------------------------------------------------------------ the assembled decoder
import copy                                                                               # noqa: E402

from proxytransformation_amd import GroundingLoss                                         # noqa: E402
from tests import decoder_util as du                                                      # noqa: E402
from tests import query_select_util as qu                                                 # noqa: E402
from tests.test_gpu_decoder import count_synchronises                                     # noqa: E402

INPUT_LEAVES = ("query", "key", "text_feats")


def call(m, t, branches):
    return m(t["query"], t["key"], t["key"], t["key_padding_mask"], None, None, t["query_coords"], t["key_coords"], t["pred_bboxes"],
             t["text_feats"], t["text_attention_mask"], branches)


def device_step(name):
    """One training step of the case on the device: the forward's results, every gradient under the twin's names, the buffers."""
    m, branches, ops, G = tu.dec_setup(name)
    md, bd = copy.deepcopy(m).to(DEV).train(), copy.deepcopy(branches).to(DEV).train()
    t = {k: dev(v, k in INPUT_LEAVES) for k, v in ops.items()}
    out = call(md, t, bd)
    sum((o * dev(g)).sum() for o, g in zip(out, G)).backward()
    grads = {n: host(p.grad) for n, p in md.named_parameters() if p.grad is not None}
    grads.update({f"reg.{lid}.{n}": host(p.grad) for lid, br in enumerate(bd) for n, p in br.named_parameters() if p.grad is not None})
    grads.update({k: host(t[k].grad) for k in INPUT_LEAVES})
    for k in ("key_coords", "query_coords", "pred_bboxes"):
        assert t[k].grad is None
    return dict(out=tuple(host(o) for o in out), grads=grads, buffers={n: host(b) for n, b in md.named_buffers()})


@pytest.mark.parametrize("name", ["small", "tk", "groups", "last", "shifted", "notoken"])
def test_decoder_training_step_against_the_train_mode_twin(name):
    """Forward results, every parameter's gradient and ``dquery``, ``dkey``, ``dtext`` by ``hold`` against the float64 train-mode torch
    twin (the fp32 twin on the CPU is the yardstick), the three leaves that are zero in exact arithmetic by their bounds; the running
    statistics and counters of both position embeddings after the step."""
    m, branches, ops, G = tu.dec_setup(name)
    r32, r64 = tu.dec_refs(name)
    got = device_step(name)
    NL = m.num_layers
    for i, o in enumerate(got["out"]):
        su.hold(f"decoder {name} out{i}", o, r32["out"][i], r64["out"][i])
    assert set(got["grads"]) == set(r64["grads"]), set(got["grads"]) ^ set(r64["grads"])
    assert not any(".self_posembed." in n and n.startswith("layers.") for n in got["grads"])      # constructed, never called
    bounds = tu.zero_leaf_bounds(m, r64, ops["query"].shape[1])
    small = []
    for n in sorted(got["grads"]):
        g = got["grads"][n]
        assert g.shape == r64["grads"][n].shape and g.dtype == np.float32 and np.isfinite(g).all(), n
        if n in tu.ZERO_LEAVES:
            weight = n.rsplit(".", 1)[0] + ".weight"
            print(f"decoder {name} {n}: |gpu| {np.abs(g).max():.3e}  bound {bounds[n].max():.3e}  |{weight}| {np.abs(r64['grads'][weight]).max():.3e}")
            assert (np.abs(g) <= bounds[n]).all(), (n, float(np.abs(g).max()), float(bounds[n].max()))
        elif g.size < su.MIN_SAMPLE:
            small.append(n)
        else:
            su.hold(f"decoder {name} {n}", g, r32["grads"][n], r64["grads"][n])
    if small:                                                # the 9-value biases of the regression branches, pooled over the layers
        cat = lambda r: np.concatenate([r[n].ravel() for n in small])      # noqa: E731
        su.hold(f"decoder {name} {'+'.join(small)}", cat(got["grads"]), cat(r32["grads"]), cat(r64["grads"]))
    for n, ref in r64["buffers"].items():
        if n.endswith("num_batches_tracked"):
            assert int(got["buffers"][n]) == int(ref) == NL, n
        else:
            su.hold(f"decoder {name} {n}", got["buffers"][n], r32["buffers"][n], ref)


def test_decoder_eval_bits_survive_a_training_step_and_two_steps_agree():
    """Without the keyword nothing changes: the eval forward of SMALL gives the same bits before a training step and after it, once the
    parameters and buffers are restored; the flag in eval under ``no_grad`` is that same path.  Two training steps from the same state
    give the same bits; forward plus backward never synchronise."""
    m, branches, ops, G = tu.dec_setup("small")
    plain = du.module(**du.SMALL).to(DEV)                    # no keyword
    plain.load_state_dict(m.state_dict())
    bd = copy.deepcopy(branches).to(DEV).eval()
    with torch.no_grad():
        before = [host(o) for o in du.device(plain, ops, bd)]
    md = copy.deepcopy(m).to(DEV)
    state = copy.deepcopy(md.state_dict())
    with torch.no_grad():
        flagged = [host(o) for o in du.device(md.eval(), ops, bd)]
    assert all(bits_equal(a, b) for a, b in zip(before, flagged))
    md.train()
    t = {k: dev(v, k in INPUT_LEAVES) for k, v in ops.items()}
    sum((o * dev(g)).sum() for o, g in zip(call(md, t, bd), G)).backward()
    assert int(md.cross_posembed.position_embedding_head[1].num_batches_tracked) == m.num_layers
    md.load_state_dict(state)
    with torch.no_grad():
        after = [host(o) for o in du.device(md.eval(), ops, bd)]
    assert all(bits_equal(a, b) for a, b in zip(before, after))
    with pytest.raises(NotImplementedError, match="eval forward only"):
        du.device(plain.train(), ops, bd)
    first = device_step("small")
    torch.cuda.synchronize()
    md.train()
    t = {k: dev(v, k in INPUT_LEAVES) for k, v in ops.items()}
    gs = [dev(g) for g in G]
    torch.cuda.synchronize()
    with count_synchronises() as calls:
        sum((o * g).sum() for o, g in zip(call(md, t, bd), gs)).backward()
    assert calls == [], f"forward plus backward synchronised: {calls}"
    again = device_step("small")
    for n in first["grads"]:
        assert bits_equal(first["grads"][n], again["grads"][n]), n
    assert all(bits_equal(a, b) for a, b in zip(first["out"], again["out"]))


def test_decoder_refusals_come_before_any_launch():
    m, branches, ops, G = tu.dec_setup("small")
    md, bd = copy.deepcopy(m).to(DEV).eval(), copy.deepcopy(branches).to(DEV)
    state = {k: host(v).copy() for k, v in md.state_dict().items()}
    t = {k: dev(v, k == "query") for k, v in ops.items()}
    with pytest.raises(NotImplementedError, match="frozen BatchNorm"):
        call(md, t, bd)
    md.train()
    with pytest.raises(NotImplementedError, match="cross_attn_mask"):
        md(t["query"], t["key"], t["key"], t["key_padding_mask"], None, torch.zeros(1, device=DEV), t["query_coords"], t["key_coords"],
           t["pred_bboxes"], t["text_feats"], t["text_attention_mask"], bd)
    with pytest.raises(NotImplementedError, match="value must be key"):
        md(t["query"], t["key"], t["key"].clone(), t["key_padding_mask"], None, None, t["query_coords"], t["key_coords"], t["pred_bboxes"],
           t["text_feats"], t["text_attention_mask"], bd)
    assert all(np.array_equal(host(v), state[k]) for k, v in md.state_dict().items())      # no running statistic moved
    empty = dict(t, query=t["query"][:, :0], query_coords=t["query_coords"][:, :0], pred_bboxes=t["pred_bboxes"][:, :0])
    hidden, boxes = call(md, empty, bd)                      # K == 0: the shaped zeros, no launch, also in training
    assert tuple(hidden.shape) == (m.num_layers, 2, 0, m.embed_dims) and tuple(boxes.shape) == (m.num_layers, 2, 0, 9)
    assert all(np.array_equal(host(v), state[k]) for k, v in md.state_dict().items())


# ------------------------------------------------------------------------------------------------------------------ end to end
E2E_ROWS, E2E_K, E2E_DEC = (200, 90, 130), 64, dict(C=256, heads=8, ffn=256, layers=2)


def e2e_step():
    """``QuerySelect(differentiable=True)`` -> decoder -> ``head_scores(differentiable=True)`` -> ``GroundingLoss.loss`` -> sum ->
    backward on a cut of the end-to-end inputs (the first 200 / 90 / 130 rows of the three scenes, 64 queries, two layers)."""
    feats, xyz, text, mask = qu.e2e_inputs()
    qs = qu.module(num_queries=E2E_K, differentiable=True).to(DEV)
    dec = du.module(**E2E_DEC, differentiable=True).to(DEV).train()
    f = [dev(a[:n], True) for a, n in zip(feats, E2E_ROWS)]
    x = [dev(a[:n]) for a, n in zip(xyz, E2E_ROWS)]
    text_t, token_mask = dev(text, True), dev(mask)
    d, head = qs(f, None, x, text_t, token_mask)
    d["query"].retain_grad()
    d["feats"].retain_grad()
    hidden, boxes = dec(d["query"], d["feats"], d["feats"], d["feats_attention_mask"], None, None, d["query_coords"], d["feats_coords"],
                        d["pred_bboxes"], d["text_feats"], d["text_attention_mask"], qs)
    hidden.retain_grad()
    boxes.retain_grad()
    scores = dec.head_scores(hidden, head, qs, differentiable=True)
    scores.retain_grad()
    rng = np.random.default_rng(32)
    gts, pms = [], []
    for b, g in enumerate((2, 1, 3)):
        gt = host(boxes)[-1, b, :g] + rng.normal(0, 0.05, (g, 9))
        gt[:, 3:6] = np.abs(gt[:, 3:6]) + 0.05
        gts.append(dev(gt.astype(np.float32)))
        pm = np.zeros((g, qs.max_text_len), np.float32)
        pm[:, np.nonzero(mask[b])[0][:2]] = 0.5
        pms.append(dev(pm))
    out = GroundingLoss().loss(scores, boxes, token_mask, gts, pms)
    sum(out.values()).backward()
    return dict(qs=qs, dec=dec, feats=f, text=text_t, d=d, hidden=hidden, boxes=boxes, scores=scores, mask=mask)


def test_end_to_end_every_leaf_receives_a_gradient_and_the_chain_holds():
    a = e2e_step()
    qs, dec = a["qs"], a["dec"]
    leaves = {f"feats[{b}]": t for b, t in enumerate(a["feats"])}
    leaves.update(text=a["text"], cls_bias=qs.cls_branch.bias)
    leaves.update({f"reg.{n}": p for n, p in qs.reg_branch.named_parameters()})
    leaves.update({n: p for n, p in dec.named_parameters() if not (n.startswith("layers.") and ".self_posembed." in n)})
    for n, t in leaves.items():
        assert t.grad is not None and bool(torch.isfinite(t.grad).all()) and bool(t.grad.abs().max() > 0), n
    b = e2e_step()                                           # a second run: the same bits
    leaves_b = {f"feats[{i}]": t for i, t in enumerate(b["feats"])}
    leaves_b.update(text=b["text"], cls_bias=b["qs"].cls_branch.bias)
    leaves_b.update({n: p for n, p in b["dec"].named_parameters() if n in leaves})
    for n, t in leaves_b.items():
        assert bits_equal(host(t.grad), host(leaves[n].grad)), n
    # what the loss handed to the decoder's outputs, pushed through the float64 specification of the whole chain
    # (decoder_grad_host.decoder_train_host, and scores_bwd_host for the text's share): the device's gradients of the decoder's inputs
    d = a["d"]
    ops = dict(query=host(d["query"]), key=host(d["feats"]), key_padding_mask=host(d["feats_attention_mask"]),
               query_coords=host(d["query_coords"]), key_coords=host(d["feats_coords"]), pred_bboxes=host(d["pred_bboxes"]),
               text_feats=host(d["text_feats"]), text_attention_mask=host(d["text_attention_mask"]))
    ds = host(a["scores"].grad)
    sc = {dt: tu.gh.scores_bwd_host(host(a["hidden"]).astype(dt), ops["text_feats"].astype(dt), a["mask"], ds.astype(dt), qs.has_bias, qs.scaled)
          for dt in (np.float32, np.float64)}
    cpu = du.module(**E2E_DEC, differentiable=True).train()
    branches = [copy.deepcopy(qs.reg_branch).cpu()] * E2E_DEC["layers"]
    refs = {}
    for dt in (np.float32, np.float64):                      # the fp32 torch twin on the CPU: the yardstick; the float64 specification
        G = (host(a["hidden"].grad).astype(dt), host(a["boxes"].grad).astype(dt))
        grads = tu.train_twin_step(cpu, branches, ops, G, torch.float32)["grads"] if dt == np.float32 else tu.spec_step(cpu, branches, ops, G)[1]
        refs[dt] = dict(query=grads["query"], key=grads["key"], text=grads["text_feats"] + sc[dt]["dtext"])
    # hidden reaches the loss through the scores alone, so hidden.grad as retained is the scores' dhidden
    got = dict(query=host(d["query"].grad), key=host(d["feats"].grad), text=host(a["text"].grad))
    for n in got:
        su.hold(f"end to end d{n}", got[n], refs[np.float32][n], refs[np.float64][n])
