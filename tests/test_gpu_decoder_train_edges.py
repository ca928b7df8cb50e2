"""The decoder's training operators (csrc/decoder_train.hip) at the sizes tests/test_gpu_decoder_train.py does not draw, by that
module's rules (``sparse_util.hold`` against float64 torch with the fp32 CPU chain as the yardstick; tests/test_decoder_train_host.py
asserts the yardstick's precondition on every case drawn here):

  * the row-slab reductions beyond their first slab -- ``k_pe_moments`` / ``k_pe_fold`` (Chan's merge over slabs), ``k_dec_slab`` in
    its three modes and ``k_dec_slab_finish`` with S = 2, 3 and 513 -- and with two chunks per slab (262145 rows: the ``ci >= 1``
    iterations, the merge between chunks, the ``break`` on a chunk behind the end);
  * ``ptx_dec_scores_bwd`` beyond one channel tile (``col0 > 0``), at exact K and T tiles and at the admitted limits of K and T;
  * ``boxes(differentiable=True)`` with ``bias=None``.

The 262145-row case alone goes by ``decoder_train_util.hold_ratio_capped`` (decoder_train_util says why, with the figures)."""
import numpy as np
import pytest
import torch

from proxytransformation_amd import decoder
from tests import decoder_train_util as tu
from tests import sparse_util as su
from tests import test_gpu_decoder_train as base
from tests.test_gpu_decoder import count_synchronises

pytestmark = pytest.mark.gpu
DEV = su.DEV
dev, host, bits_equal = base.dev, base.host, base.bits_equal
run_posembed, run_boxes, run_scores = base.run_posembed, base.run_boxes, base.run_scores
PE_HELD = ("out", "running_mean", "running_var") + tuple(g for g in tu.PE_GRADS if g != "dconv1_b")


def same_bits(a, b):
    for k in a:
        assert k == "num_batches_tracked" or bits_equal(a[k], b[k]), k


def hold_bias_bound(name, c, got, r64):
    bound = tu.conv1_bias_bound(c)
    print(f"{name} dconv1_b: |gpu| {np.abs(got['dconv1_b']).max():.3e}  bound {bound.max():.3e}  |dconv1_w| {np.abs(r64['dconv1_w']).max():.3e}")
    assert (np.abs(got["dconv1_b"]) <= bound).all(), (name, float(np.abs(got["dconv1_b"]).max()), float(bound.max()))


# ------------------------------------------------------------------------------------------------------------------ posembed
@pytest.mark.parametrize("cin,C,n,shift,padded", tu.PE_SLAB_CASES)
def test_posembed_over_several_slabs(cin, C, n, shift, padded):
    """S = 2 and 3: the results, both running statistics, the counter and the gradients as the one-slab cases are held; the forward's
    bits are the plain launch on ``posembed_folded``'s operands; two runs give the same bits."""
    base.test_posembed_training_forward_statistics_and_gradients(cin, C, n, shift, padded)
    c = tu.pe_case(cin, C, n, shift, padded)
    folded = decoder.posembed_folded(dev(c["x"]), tu.pe_module(c, dev=DEV))
    with torch.no_grad():
        plain = decoder.posembed(dev(c["x"]), folded)
    a, b = run_posembed(c), run_posembed(c)
    assert bits_equal(host(plain), a["out"])
    same_bits(a, b)


def test_posembed_with_two_chunks_per_slab():
    """262145 rows: 1025 chunks, two per slab, 513 slabs, the last of one row.  Every leaf by ``hold_ratio`` and at most 8e-5 off
    float64; ``dconv1_b`` inside ``conv1_bias_bound`` (the fp32 torch chain's own value, printed, is no yardstick at this size: its float
    row sum misses the bound); the counter; two runs give the same bits."""
    case = tu.PE_CHUNK_CASE
    c = tu.pe_case(*case)
    r32, r64 = tu.pe_refs(*case)
    got = run_posembed(c, repeat=1)
    assert got["num_batches_tracked"] == r64["num_batches_tracked"] == 6
    name = f"posembed n={case[2]}"
    for k in PE_HELD:
        assert got[k].shape == r64[k].shape and got[k].dtype == np.float32, k
        tu.hold_ratio_capped(f"{name} {k}", got[k], r32[k], r64[k])
    print(f"{name} dconv1_b: fp32 torch {np.abs(r32['dconv1_b']).max():.3e} (no yardstick here)")
    hold_bias_bound(name, c, got, r64)
    same_bits(got, run_posembed(c, repeat=1))


def test_posembed_slab_boundary_and_row_order():
    """The first 256 rows of the 257-row case alone are one slab; with the 257th they are two.  Reversing the order of rows 0..255 of
    ``x`` and ``dout`` changes nothing in exact arithmetic (``out`` comes back reversed): on either side of the boundary the device's
    results of both orders satisfy ``hold`` against the SAME float64 reference."""
    case = tu.PE_SLAB_CASES[0]
    whole = tu.pe_case(*case)
    cut = tu.pe_cut(whole, 256)
    for label, c, (r32, r64) in (("256 rows", cut, (tu.pe_torch(cut, torch.float32), tu.pe_torch(cut, torch.float64))),
                                 ("257 rows", whole, tu.pe_refs(*case))):
        for order, cc in (("as drawn", c), ("reversed", tu.pe_reversed(c, 256))):
            got = run_posembed(cc)
            if order == "reversed":
                got["out"][:, :256] = got["out"][:, :256][:, ::-1].copy()
            assert got["num_batches_tracked"] == 6
            for k in PE_HELD:
                su.hold(f"posembed {label} {order} {k}", got[k], r32[k], r64[k])
            hold_bias_bound(f"posembed {label} {order}", c, got, r64)


# ------------------------------------------------------------------------------------------------------------------ boxes
@pytest.mark.parametrize("C,n", tu.BOX_SLAB_CASES)
def test_boxes_over_several_slabs(C, n):
    """``dW = dp^T h`` with S = 2 and 3, as the one-slab cases are held: both sides of the clamp, the plain call's forward bits, ``dh``
    and ``dweight`` by ``hold``, ``dbias`` pooled."""
    base.test_boxes_gradients_on_both_sides_of_the_clamp(C, n)


def test_boxes_without_a_bias():
    C, n = tu.BOX_NOBIAS_CASE
    c = tu.box_case(C, n, has_bias=False)
    r32, r64 = tu.box_refs(C, n, has_bias=False)
    h, w = dev(c["h"], True), dev(c["weight"], True)
    out = decoder.boxes(h, w, None, dev(c["coords"]), differentiable=True)
    with torch.no_grad():
        plain = decoder.boxes(dev(c["h"]), dev(c["weight"]), None, dev(c["coords"]))
    assert bits_equal(host(out), host(plain))
    sizes = host(out)[..., 3:6]
    assert (sizes == np.float32(0.02)).any() and (sizes > np.float32(0.02)).any()      # both sides of the clamp
    # the node's tensor inputs are (h, weight, coords) -- the absent bias is none: exactly three gradients, to (h, weight, nothing)
    edges = out.grad_fn.next_functions
    assert len(edges) == 3 and edges[0][0] is not None and edges[1][0] is not None and edges[2][0] is None
    grads = torch.autograd.grad(out, (h, w), dev(c["dboxes"]))
    assert len(grads) == 2
    for k, g in zip(("dh", "dweight"), grads):
        g = host(g)
        assert g.shape == r64[k].shape and g.dtype == np.float32
        su.hold(f"boxes without a bias C={C} n={n} {k}", g, r32[k], r64[k])


# ------------------------------------------------------------------------------------------------------------------ scores
@pytest.mark.parametrize("NL,B,K,T,M,C", tu.SCORE_WIDE_CASES)
def test_scores_gradients_at_width(NL, B, K, T, M, C):
    for scaled, has_bias in ((True, True), (False, False)):
        c = tu.score_case(NL, B, K, T, M, C=C)
        out, got = run_scores(c, scaled, has_bias)
        with torch.no_grad():
            plain = decoder.contrastive_scores(dev(c["hidden"]), dev(c["text"]), dev(c["mask"]), dev(c["bias"]) if has_bias else None, scaled, M)
        assert bits_equal(host(out), host(plain))
        assert ("dbias" in got) == has_bias
        r32, r64 = tu.score_torch(c, torch.float32, scaled, has_bias), tu.score_torch(c, torch.float64, scaled, has_bias)
        for k in ("dhidden", "dtext"):
            assert got[k].shape == r64[k].shape and got[k].dtype == np.float32
            su.hold(f"scores {NL, B, K, T, M, C} scaled={scaled} {k}", got[k], r32[k], r64[k])
        assert not got["dtext"][~c["mask"]].view(np.uint32).any()      # bit zero on a masked token
    seeds = iter(range(200))
    su.hold_pooled(f"scores {NL, B, K, T, M, C} dbias", 1, lambda: (tu.score_case(NL, B, K, T, M, next(seeds), C=C),),
                   lambda c: run_scores(c)[1]["dbias"], lambda c: (tu.score_torch(c, torch.float32)["dbias"], tu.score_torch(c, torch.float64)["dbias"]))


def test_scores_a_nan_under_the_mask_or_behind_T_leaves_no_trace_at_width():
    """Four channel tiles, one scene with every token masked: NaN under every masked token and from column T on leaves ``dhidden``,
    ``dtext`` and ``dbias`` finite and bit for bit those of the clean gradient."""
    NL, B, K, T, M, C = tu.SCORE_WIDE_CASES[0]
    c = tu.score_case(NL, B, K, T, M, all_masked_scene=True, C=C)
    _, clean = run_scores(c)
    d = c["dscores"].copy()
    d[..., T:] = np.nan
    d[..., :T][np.broadcast_to(~c["mask"][None, :, None, :], d[..., :T].shape)] = np.nan
    _, dirty = run_scores(dict(c, dscores=d))
    r32, r64 = tu.score_torch(c, torch.float32), tu.score_torch(c, torch.float64)
    for k in clean:
        assert np.isfinite(dirty[k]).all() and bits_equal(clean[k], dirty[k]), k
    for k in ("dhidden", "dtext"):
        su.hold(f"scores at C={C} with a scene without tokens {k}", clean[k], r32[k], r64[k])
    assert not clean["dhidden"][:, -1].view(np.uint32).any() and not clean["dtext"][-1].view(np.uint32).any()


# ------------------------------------------------------------------------------------------------------------------ no wait, same bits
def test_slab_and_wide_launches_never_synchronise_and_repeat_their_bits():
    cb = tu.box_case(*tu.BOX_SLAB_CASES[1])
    NL, B, K, T, M, C = tu.SCORE_WIDE_CASES[3]
    cs = tu.score_case(NL, B, K, T, M, C=C)
    tb = {k: dev(cb[k], k in ("h", "weight", "bias")) for k in ("h", "weight", "bias", "coords", "dboxes")}
    hs, text, bias = dev(cs["hidden"], True), dev(cs["text"], True), dev(cs["bias"], True)
    mask, ds = dev(cs["mask"]), dev(cs["dscores"])
    torch.cuda.synchronize()
    with count_synchronises() as calls:
        (decoder.boxes(tb["h"], tb["weight"], tb["bias"], tb["coords"], differentiable=True) * tb["dboxes"]).sum().backward()
        decoder.contrastive_scores(hs, text, mask, bias, True, M, differentiable=True).backward(ds)
    assert calls == [], f"forward plus backward synchronised: {calls}"
    first = dict(dh=host(tb["h"].grad), dweight=host(tb["weight"].grad), dbias=host(tb["bias"].grad))
    again = run_boxes(cb)[1]
    for k in first:
        assert bits_equal(first[k], again[k]), k
    first = dict(dhidden=host(hs.grad), dtext=host(text.grad), dbias=host(bias.grad))
    again = run_scores(cs)[1]
    for k in first:
        assert bits_equal(first[k], again[k]), k
