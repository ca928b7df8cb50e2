"""The numpy specification of the decoder's training operators (proxytransformation_amd/decoder_grad_host.py: the position embedding with
batch statistics, forward and backward; the box head's backward; the text scores' backward) against float64 torch autograd at 1e-10 and,
where the function is smooth, against central differences; the running-statistics rule against ``nn.BatchNorm1d``; the yardsticks and
the bound that tests/test_gpu_decoder_train.py relies on; the ABI surface.  Runs without a GPU."""
import math

import numpy as np
import pytest
import torch

from proxytransformation_amd import decoder, decoder_grad_host as gh
from tests import decoder_train_util as tu
from tests import sparse_util as su


def close(a, b, tol=1e-10):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and float(np.abs(a - b).max()) <= tol * max(1.0, float(np.abs(b).max()))


# ------------------------------------------------------------------------------------------------------------------ posembed
@pytest.mark.parametrize("cin,n", [(3, 2), (9, 2), (3, 130), (9, 130)])
@pytest.mark.parametrize("shift", [0.0, 100.0])
@pytest.mark.parametrize("repeat", [1, 3])
def test_posembed_training_specification_is_torch(cin, n, shift, repeat):
    c = tu.pe_case(cin, 64, n, shift, seed=1)                # unit spread, no padding
    ref, spec = tu.pe_torch(c, torch.float64, repeat), tu.pe_spec(c, np.float64, repeat)
    for k in ("out", "running_mean", "running_var") + tu.PE_GRADS:
        assert close(spec[k], ref[k]), k
    assert ref["num_batches_tracked"] == 5 + repeat          # what the operator adds to the counter


def test_posembed_specification_against_central_differences():
    """The loss ``sum(out * dout)`` as a function of each parameter, float64, steps of 1e-6 at a handful of entries."""
    c = {k: tu.f64(v) for k, v in tu.pe_case(3, 64, 130, 0.0, seed=2).items()}
    names = dict(dconv1_w="conv1_w", dconv1_b="conv1_b", dbn_w="bn_w", dbn_b="bn_b", dconv2_w="conv2_w", dconv2_b="conv2_b")
    grads = gh.posembed_train_bwd_host(c["x"], c["conv1_w"], c["conv1_b"], c["bn_w"], c["bn_b"], c["conv2_w"], c["dout"], tu.BN_EPS)

    def loss(p):
        out = gh.posembed_train_host(c["x"], p["conv1_w"], p["conv1_b"], p["bn_w"], p["bn_b"], p["conv2_w"], p["conv2_b"], tu.BN_EPS)[0]
        return float((out * c["dout"]).sum())

    rng = np.random.default_rng(3)
    for g, name in names.items():
        for _ in range(3):
            at = tuple(int(rng.integers(0, s)) for s in c[name].shape)
            hi, lo = {k: v.copy() for k, v in c.items()}, {k: v.copy() for k, v in c.items()}
            hi[name][at] += 1e-6
            lo[name][at] -= 1e-6
            num = (loss(hi) - loss(lo)) / 2e-6
            got = grads[g][at[:grads[g].ndim]]
            assert abs(num - got) <= 1e-5 * max(1.0, abs(got)), (g, at, num, got)


def test_posembed_one_row_is_refused_as_torch_refuses_it():
    c = tu.pe_case(3, 64, 2, 0.0)
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        gh.posembed_train_host(c["x"][:, :1], c["conv1_w"], c["conv1_b"], c["bn_w"], c["bn_b"], c["conv2_w"], c["conv2_b"])
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        tu.pe_module(c)(torch.from_numpy(c["x"][:, :1]).transpose(1, 2))


@pytest.mark.parametrize("cin,C,n,shift,padded", tu.PE_SLAB_CASES + [tu.PE_CHUNK_CASE])
def test_posembed_specification_is_torch_over_several_slabs(cin, C, n, shift, padded):
    """The cases of tests/test_gpu_decoder_train_edges.py: the numpy specification is the float64 torch chain at 1e-10 on each.  At
    262145 rows no leaf goes by ``hold``, so no precondition is asserted there: the fp32 chain's yardsticks and its ``dconv1_b`` against
    the bound are printed (fp32 torch is no yardstick for that leaf at this size, decoder_train_util says why), and float64's own
    ``dconv1_b`` is at rounding scale."""
    c = tu.pe_case(cin, C, n, shift, padded)
    r32, r64 = tu.pe_refs(cin, C, n, shift, padded)
    spec = tu.pe_spec(c, np.float64)
    for k in ("out", "running_mean", "running_var") + tu.PE_GRADS:
        if k == "dconv1_b":                                  # zero in exact arithmetic: both are roundings, at the scale of dconv1_w's terms
            assert float(np.abs(spec[k] - r64[k]).max()) <= 1e-10 * max(1.0, float(np.abs(r64["dconv1_w"]).max())), k
            continue
        assert close(spec[k], r64[k]), k
    assert r64["num_batches_tracked"] == 6
    if (cin, C, n, shift, padded) == tu.PE_CHUNK_CASE:
        for k in ("out", "running_mean", "running_var") + tuple(g for g in tu.PE_GRADS if g != "dconv1_b"):
            print(f"posembed {n} rows {k}: fp32 yardstick {su.rel(r32[k], r64[k]):.3e}")
        bound = tu.conv1_bias_bound(c)
        print(f"posembed {n} rows dconv1_b: fp32 torch {np.abs(r32['dconv1_b']).max():.3e}  float64 {np.abs(r64['dconv1_b']).max():.3e}  "
              f"bound {bound.max():.3e}  |dconv1_w| {np.abs(r64['dconv1_w']).max():.3e}")
        assert np.isfinite(bound).all() and (bound > 0).all()
        assert float(np.abs(r64["dconv1_b"]).max()) <= 1e-9 * max(1.0, float(np.abs(r64["dconv1_w"]).max()))


def test_posembed_first_slab_alone_and_reversed_rows():
    """The first 256 rows of the 257-row case alone (one slab): ``hold``'s precondition and the bound on that cut, which the GPU module
    draws; reversing the order of those rows moves nothing in float64 but the order of ``out``."""
    case = tu.PE_SLAB_CASES[0]
    c = tu.pe_cut(tu.pe_case(*case), 256)
    r32, r64 = tu.pe_torch(c, torch.float32), tu.pe_torch(c, torch.float64)
    back = tu.pe_torch(tu.pe_reversed(c, 256), torch.float64)
    for k in ("out", "running_mean", "running_var") + tuple(g for g in tu.PE_GRADS if g != "dconv1_b"):
        assert su.rel(r32[k], r64[k]) < 1e-5, (k, su.rel(r32[k], r64[k]))
        assert close(back[k][:, ::-1] if k == "out" else back[k], r64[k]), k
    assert (np.abs(r32["dconv1_b"]) <= tu.conv1_bias_bound(c)).all()
    whole = tu.pe_reversed(tu.pe_case(*case), 256)
    assert np.array_equal(whole["x"][:, 256:], tu.pe_case(*case)["x"][:, 256:]) and np.array_equal(whole["x"][:, 255], tu.pe_case(*case)["x"][:, 0])


@pytest.mark.parametrize("cin,C,n,shift,padded", tu.PE_CASES + tu.PE_SLAB_CASES + [tu.PE_UNPADDED])
def test_posembed_yardsticks_and_the_bias_bound(cin, C, n, shift, padded):
    """``hold``'s precondition on every case the GPU module draws (the fp32 CPU torch chain within 1e-5 of float64), and the fp32 torch
    chain's own ``dconv1_b`` inside the bound the device is held to: the bound is not fitted to the device."""
    c = tu.pe_case(cin, C, n, shift, padded)
    r32, r64 = tu.pe_refs(cin, C, n, shift, padded)
    for k in ("out", "running_mean", "running_var") + tuple(g for g in tu.PE_GRADS if g != "dconv1_b"):
        if (cin, C, n, shift, padded) == tu.PE_UNPADDED:     # decoder_train_util says why: the ratio alone
            assert su.rel(r32[k], r64[k]) < (1e-2 if k == "dconv1_w" else 1e-4), k
            continue
        assert r32[k].dtype == np.float32 and su.rel(r32[k], r64[k]) < 1e-5, (k, su.rel(r32[k], r64[k]))
    bound = tu.conv1_bias_bound(c)
    print(f"posembed {cin, C, n, shift, padded} dconv1_b: fp32 torch {np.abs(r32['dconv1_b']).max():.3e}  float64 {np.abs(r64['dconv1_b']).max():.3e}  "
          f"bound {bound.max():.3e}  |dconv1_w| {np.abs(r64['dconv1_w']).max():.3e}")
    assert (np.abs(r32["dconv1_b"]) <= bound).all()
    assert float(np.abs(r64["dconv1_b"]).max()) <= 1e-9 * max(1.0, float(np.abs(r64["dconv1_w"]).max()))


# ------------------------------------------------------------------------------------------------------------------ boxes
def test_boxes_specification_is_torch_on_both_sides_of_the_clamp():
    for C, n in tu.BOX_CASES + tu.BOX_SLAB_CASES:
        c = tu.box_case(C, n)
        ref = tu.box_torch(c, torch.float64)
        spec = gh.boxes_bwd_host(tu.f64(c["h"]), tu.f64(c["weight"]), tu.f64(c["bias"]), tu.f64(c["dboxes"]))
        p = tu.f64(c["h"]).reshape(n, C) @ tu.f64(c["weight"]).T + tu.f64(c["bias"])
        if n >= 17:
            assert (p[:, 3:6] > tu.LOG_CLAMP).any() and (p[:, 3:6] < tu.LOG_CLAMP).any()
        for k in ("dh", "dweight", "dbias"):
            assert close(spec[k], ref[k]), (C, n, k)
        r32 = tu.box_torch(c, torch.float32)
        for k in ("dh", "dweight", "dbias"):
            assert su.rel(r32[k], ref[k]) < 1e-5, (C, n, k)


def test_boxes_specification_is_torch_without_a_bias():
    """``bias=None``: the draw's log-sizes still lie on both sides of the clamp (``h`` scaled, decoder_train_util), the specification
    returns no ``dbias`` and is float64 torch, and ``hold``'s precondition holds for ``dh`` and ``dweight``."""
    C, n = tu.BOX_NOBIAS_CASE
    c = tu.box_case(C, n, has_bias=False)
    assert c["bias"] is None
    r32, ref = tu.box_refs(C, n, has_bias=False)
    spec = gh.boxes_bwd_host(tu.f64(c["h"]), tu.f64(c["weight"]), None, tu.f64(c["dboxes"]))
    p = tu.f64(c["h"]).reshape(n, C) @ tu.f64(c["weight"]).T
    assert (p[:, 3:6] > tu.LOG_CLAMP + 1e-3).any() and (p[:, 3:6] < tu.LOG_CLAMP - 1e-3).any()
    assert np.abs(p[:, 3:6] - tu.LOG_CLAMP).min() > 1e-3
    assert set(spec) == {"dh", "dweight"} and "dbias" not in ref
    for k in ("dh", "dweight"):
        assert close(spec[k], ref[k]), k
        print(f"boxes without a bias {k}: fp32 yardstick {su.rel(r32[k], ref[k]):.3e}")
        assert su.rel(r32[k], ref[k]) < 1e-5, k


def test_boxes_on_the_clamp_nan_and_infinities():
    """A log-size exactly on the clamp passes its gradient (``exp(p) >= 0.02``); a NaN gives NaN, ``+inf`` gives ``d * inf``, ``-inf`` 0:
    what torch's float64 autograd gives for ``exp(p).clamp(min=0.02)``."""
    on = math.log(0.02)
    assert math.exp(on) == 0.02 and float(torch.exp(torch.tensor(on, dtype=torch.float64))) == 0.02
    below = float(np.nextafter(on, -np.inf))
    h, w, d = np.zeros((1, 1, 64)), np.zeros((9, 64)), np.full((1, 1, 9), 2.0)
    want = {on: 2.0 * 0.02, np.nan: np.nan, np.inf: np.inf, -np.inf: 0.0, below: 0.0, 1.0: 2.0 * math.exp(1.0)}
    for val, expect in want.items():                         # p[0, 3] = bias[3] = val; dbias[3] = dp[0, 3]
        bias = np.zeros(9)
        bias[3] = val
        got = gh.boxes_bwd_host(h, w, bias, d)["dbias"]
        t = torch.from_numpy(bias).requires_grad_()
        p = torch.from_numpy(h) @ torch.from_numpy(w).T + t
        out = torch.cat([p[..., :3], torch.exp(p[..., 3:6]).clamp(min=2e-2), p[..., 6:]], -1)
        (out * torch.from_numpy(d)).sum().backward()
        assert np.array_equal(got, t.grad.numpy(), equal_nan=True), val
        assert np.array_equal(got[3], expect, equal_nan=True) and (np.delete(got, 3) == 2.0).all(), (val, got)


# ------------------------------------------------------------------------------------------------------------------ scores
@pytest.mark.parametrize("NL,B,K,T,M", tu.SCORE_CASES)
@pytest.mark.parametrize("scaled", [True, False])
@pytest.mark.parametrize("has_bias", [True, False])
def test_scores_specification_is_torch(NL, B, K, T, M, scaled, has_bias):
    c = tu.score_case(NL, B, K, T, M)
    ref, spec = tu.score_torch(c, torch.float64, scaled, has_bias), tu.score_spec(c, np.float64, scaled, has_bias)
    assert set(ref) == set(spec)
    for k in ref:
        assert close(spec[k], np.asarray(ref[k]).reshape(np.shape(spec[k]))), k
    assert not spec["dtext"][~c["mask"]].any()               # a masked token gets zeros


@pytest.mark.parametrize("NL,B,K,T,M,C", tu.SCORE_WIDE_CASES)
@pytest.mark.parametrize("scaled,has_bias", [(True, True), (False, False)])
def test_scores_specification_is_torch_at_width(NL, B, K, T, M, C, scaled, has_bias):
    """The cases of tests/test_gpu_decoder_train_edges.py: the specification is float64 torch, and ``hold``'s precondition."""
    c = tu.score_case(NL, B, K, T, M, C=C)
    assert c["hidden"].shape == (NL, B, K, C) and c["text"].shape == (B, T, C)
    ref, spec = tu.score_torch(c, torch.float64, scaled, has_bias), tu.score_spec(c, np.float64, scaled, has_bias)
    r32 = tu.score_torch(c, torch.float32, scaled, has_bias)
    assert set(ref) == set(spec)
    for k in ref:
        assert close(spec[k], np.asarray(ref[k]).reshape(np.shape(spec[k]))), k
    for k in ("dhidden", "dtext"):
        assert r32[k].dtype == np.float32 and su.rel(r32[k], ref[k]) < 1e-5, (k, su.rel(r32[k], ref[k]))
    assert not spec["dtext"][~c["mask"]].any()


def test_scores_never_read_the_gradient_under_the_mask_at_width():
    NL, B, K, T, M, C = tu.SCORE_WIDE_CASES[0]
    c = tu.score_case(NL, B, K, T, M, all_masked_scene=True, C=C)
    clean = tu.score_spec(c, np.float64)
    d = c["dscores"].copy()
    d[..., T:] = np.nan
    d[..., :T][np.broadcast_to(~c["mask"][None, :, None, :], d[..., :T].shape)] = np.nan
    dirty = tu.score_spec(dict(c, dscores=d), np.float64)
    for k in clean:
        assert np.isfinite(dirty[k]).all() and np.array_equal(clean[k], dirty[k]), k
    assert not clean["dhidden"][:, -1].any() and not clean["dtext"][-1].any()


def test_scores_never_read_the_gradient_under_the_mask():
    c = tu.score_case(2, 2, 65, 5, 70, all_masked_scene=True)
    clean = tu.score_spec(c, np.float64)
    d = c["dscores"].copy()
    d[..., 5:] = np.nan                                      # behind T
    d[..., :5][np.broadcast_to(~c["mask"][None, :, None, :], d[..., :5].shape)] = np.nan      # under a masked token
    dirty = tu.score_spec(dict(c, dscores=d), np.float64)
    for k in clean:
        assert np.isfinite(dirty[k]).all() and np.array_equal(clean[k], dirty[k]), k
    assert not clean["dhidden"][:, -1].any() and not clean["dtext"][-1].any()      # the scene without a token


# ------------------------------------------------------------------------------------------------------------------ surface
def test_entry_points_are_declared_everywhere():
    params = su.assert_declared(tu.ENTRY_POINTS)
    assert all("void *stream" in params[n] for n in tu.ENTRY_POINTS if n != "ptx_dec_train_workspace_bytes")


def test_workspace_sizes():
    """``ptx_dec_train_workspace_bytes``: slabs of 256-row chunks, at most 1024 of them; 0 outside the range."""
    from proxytransformation_amd import _abi
    ws = _abi.lib().ptx_dec_train_workspace_bytes
    assert ws(1, 64, 2) == 1 * 2 * 64 * 8 and ws(256, 64, 2) == 2 * 64 * 8 and ws(257, 512, 10) == 2 * 10 * 512 * 8
    assert ws(1024 * 256, 64, 1) == 1024 * 64 * 8 and ws(1024 * 256 + 1, 64, 1) == 513 * 64 * 8      # two chunks per slab from there on
    assert ws(1 << 24, 64, 1) == 1024 * 64 * 8
    assert ws(0, 64, 2) == 0 and ws((1 << 24) + 1, 64, 2) == 0 and ws(5, 96, 2) == 0 and ws(5, 64, 11) == 0 and ws(5, 64, 0) == 0


def test_refusals_need_no_gpu():
    """The checks that come before any device work: they raise on CPU tensors too, or say that there is no CPU path."""
    c = tu.pe_case(3, 64, 2, 0.0)
    head = tu.pe_module(c).eval()
    with pytest.raises(NotImplementedError, match="frozen BatchNorm"):
        decoder.posembed(torch.zeros(1, 4, 3), head, differentiable=True)
    with pytest.raises(NotImplementedError, match="x requires grad"):
        decoder.posembed(torch.zeros(1, 4, 3, requires_grad=True), head.train(), differentiable=True)
    with pytest.raises(ValueError, match="out cannot be given"):
        decoder.boxes(torch.zeros(1, 4, 64), torch.zeros(9, 64), None, torch.zeros(1, 4, 3), out=torch.zeros(1, 4, 9), differentiable=True)


# ------------------------------------------------------------------------------------------------------------------ the assembled decoder
@pytest.mark.parametrize("name", ["small", "tk", "groups", "last", "shifted", "notoken"])
def test_decoder_yardsticks_and_the_zero_leaf_bounds(name):
    """On every case the GPU module runs: no NaN in the train-mode twin (a scene with every text token masked included), ``hold``'s
    precondition on every leaf that is not zero in exact arithmetic, those three at rounding scale in float64, and the fp32 CPU torch
    chain's own value inside the bound the device is held to: the bounds are not fitted to the device."""
    m, branches, ops, G = tu.dec_setup(name)
    r32, r64 = tu.dec_refs(name)
    bounds = tu.zero_leaf_bounds(m, r64, ops["query"].shape[1])
    assert set(r32["grads"]) == set(r64["grads"])
    for n, g in r64["grads"].items():
        assert np.isfinite(g).all() and np.isfinite(r32["grads"][n]).all(), n
        if n in tu.ZERO_LEAVES:
            weight = n.rsplit(".", 1)[0] + ".weight"
            print(f"decoder {name} {n}: fp32 torch {np.abs(r32['grads'][n]).max():.3e}  float64 {np.abs(g).max():.3e}  bound {bounds[n].max():.3e}  "
                  f"|{weight}| {np.abs(r64['grads'][weight]).max():.3e}")
            assert float(np.abs(g).max()) <= 1e-10 * float(np.abs(r64["grads"][weight]).max()), n
            assert (np.abs(r32["grads"][n]) <= bounds[n]).all(), n
        elif g.size >= su.MIN_SAMPLE:
            assert su.rel(r32["grads"][n], g) < 1e-5, (n, su.rel(r32["grads"][n], g))
    for i in range(2):
        assert su.rel(r32["out"][i], r64["out"][i]) < 1e-5
    for n, b in r64["buffers"].items():
        if n.endswith("num_batches_tracked"):
            assert int(b) == m.num_layers                    # cross_posembed per layer in the reference: NL calls each
        else:
            assert su.rel(r32["buffers"][n], b) < 1e-5, n


def test_decoder_flag_is_stored_and_the_modes_are_told_apart_on_the_host():
    from tests import decoder_util as du
    assert du.module(**du.SMALL).differentiable is False and du.module(**du.SMALL, differentiable=True).differentiable is True
    m, branches, ops, G = tu.dec_setup("small")
    t = {k: torch.from_numpy(v) for k, v in ops.items()}
    args = lambda q: (q, t["key"], t["key"], t["key_padding_mask"], None, None, t["query_coords"], t["key_coords"], t["pred_bboxes"],      # noqa: E731
                      t["text_feats"], t["text_attention_mask"], branches)
    plain = du.module(**du.SMALL)
    with pytest.raises(NotImplementedError, match="eval forward only"):
        plain.train()(*args(t["query"]))
    with pytest.raises(NotImplementedError, match="inference-only"):
        plain.eval()(*args(t["query"].clone().requires_grad_()))
    flagged = du.module(**du.SMALL, differentiable=True).eval()
    with pytest.raises(NotImplementedError, match="frozen BatchNorm"):
        flagged(*args(t["query"].clone().requires_grad_()))
    with pytest.raises(RuntimeError, match="no CPU path"):
        flagged.train()(*args(t["query"]))                   # past the mode checks: the training path needs the GPU


def test_slab_plan_under_the_host_sanitizers(tmp_path):
    """The host-side index arithmetic of csrc/decoder_train.hip (the slab plan and the workspace size, csrc/dec_train_plan.h) in a
    stand-alone program built with AddressSanitizer and UBSan, run on the CPU."""
    import os
    import shutil
    import subprocess
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed"
    exe = str(tmp_path / "dec_train_plan_check")
    src = os.path.join(su.ROOT, "tests", "native", "dec_train_plan_check.cpp")
    inc = os.path.join(su.ROOT, "proxytransformation_amd", "csrc")
    flags = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if "clang" not in os.path.basename(cxx):
        flags += ["-static-libasan", "-static-libubsan"]      # the runtimes inside the program: it stands alone
    subprocess.run([cxx] + flags + ["-I", inc, src, "-o", exe], check=True)
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0 and "dec_train_plan OK" in res.stdout, res.stdout + res.stderr


@pytest.mark.parametrize("name", ["small", "tk", "last", "notoken"])
def test_whole_training_chain_of_the_specification_is_the_train_mode_twin(name):
    """``decoder_grad_host.decoder_train_host`` -- the forward on batch statistics and the backward composed from the operators'
    specifications -- against the float64 train-mode torch twin: the results and every gradient at 1e-10."""
    m, branches, ops, G = tu.dec_setup(name)
    r64 = tu.dec_refs(name)[1]
    out, grads = tu.spec_step(m, branches, ops, G)
    assert all(close(a, b) for a, b in zip(out, r64["out"]))
    assert set(grads) == set(r64["grads"])
    for n, g in r64["grads"].items():
        assert close(grads[n], g), n
