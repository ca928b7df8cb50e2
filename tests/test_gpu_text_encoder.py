"""``ClipTextEncoder`` on the device against its numpy specification, and ``GroundingDetector`` with it.

Accuracy: with err(t) = max|t - f64| / max|f64| against ``forward_host(float64)`` over every row, the device must satisfy
err <= 4 x err of ``forward_host(float32)`` on every case of ``text_encoder_util.CASES`` -- the rule of tests/test_gpu_detector.py, with
the same margin for a different order of addition (the float32 chain's own error is 4e-7 .. 1.4e-6).  The committed capture of
``CLIPTextModel`` (tests/golden/clip_text_tiny.npz) is held the same way.  Measured ratios (device / float32 chain), MI355X: 0.72 to 1.31
from 20 tokens on (1.31 at the shipped width), 2.78 at the single token of the first case, where the float32 chain itself is 1.4e-7
off; 1.20 on the capture; DESIGN.md 5.20 carries the table.

Structure, bit for bit: two calls; a text alone against the text in its batch; causality; ids under masked positions; a NaN embedding
row under masked positions only (the "never read" rule); an id outside the vocabulary; a text whose token 0 is masked (the zeros rule,
against the specification); the limits.  The detector: ``input_ids=`` / ``attention_mask=`` against the encoder called by hand."""
import os

import numpy as np
import pytest
import torch

from tests import text_encoder_util as U
from tests.detector_util import PAD, inputs, make_detector

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGIN = 4.0


def _run(enc, ids, mask):
    out = enc(torch.from_numpy(ids).cuda(), None if mask is None else torch.from_numpy(mask).cuda())
    assert out.dtype == torch.float32 and out.grad_fn is None and not out.requires_grad
    return out


def _held(name, dev, f32, f64):
    ed, e32 = U.err(dev, f64), U.err(f32, f64)
    print(f"{name}: device {ed:.3e}, float32 chain {e32:.3e}, ratio {ed / e32:.2f}")
    assert np.isfinite(dev).all() and ed <= MARGIN * e32, (name, ed, e32)


# ------------------------------------------------------------------------------------------------------------------ accuracy
@pytest.mark.parametrize("case", U.CASES, ids=lambda c: "x".join(map(str, c)))
def test_device_against_forward_host_float64(case):
    C, H, I, layers, B, T, kind = case
    ref = U.reference(case)
    enc = U.build_encoder(C, H, I, layers, params=ref["params"]).cuda()
    out = _run(enc, ref["ids"], ref["mask"])
    assert tuple(out.shape) == (B, T, C)
    _held(str(case), out.cpu().numpy(), ref["f32"], ref["f64"])


def test_device_against_the_committed_capture_of_clip_text_model():
    C, H, I, layers, B, T = U.GOLDEN_SHAPE
    g = np.load(os.path.join(ROOT, "tests", "golden", "clip_text_tiny.npz"))
    enc = U.build_encoder(C, H, I, layers)
    dev = enc.cuda()
    for kind in U.GOLDEN_KINDS:
        mask = g[f"mask_{kind}"] != 0
        f32 = enc.forward_host(g["ids"], mask, dtype=np.float32)
        _held(f"golden {kind}", _run(dev, g["ids"], mask).cpu().numpy(), f32, g[f"out_{kind}"])


def test_the_longest_text_and_a_key_tile_without_a_token():
    """T = 256: four key tiles; text 0 has no token at 64 .. 127 (a whole tile is skipped), text 1 has token 0 only."""
    C, H, I, layers, B, T = 64, 1, 64, 1, 2, 256
    params, ids = U.make_params(C, I, layers, positions=T), U.make_ids(B, T)
    mask = np.ones((B, T), bool)
    mask[0, 64:128] = False
    mask[1, 1:] = False
    enc = U.build_encoder(C, H, I, layers, positions=T, params=params)
    f64, f32 = enc.forward_host(ids, mask), enc.forward_host(ids, mask, dtype=np.float32)
    _held("T=256", _run(enc.cuda(), ids, mask).cpu().numpy(), f32, f64)


# ------------------------------------------------------------------------------------------------------------------ structure
@pytest.fixture(scope="module")
def small():
    C, H, I, layers, B, T = 128, 2, 192, 2, 4, 20
    enc = U.build_encoder(C, H, I, layers).cuda()
    ids, mask = U.make_ids(B, T), U.make_mask("tail", B, T)          # text b keeps 19, 16, 13, 10 tokens
    return dict(enc=enc, ids=ids, mask=mask, out=_run(enc, ids, mask), shape=(C, H, I, layers, B, T))


def test_two_calls_give_equal_bits_and_a_text_does_not_depend_on_its_batch(small):
    enc, ids, mask = small["enc"], small["ids"], small["mask"]
    assert torch.equal(_run(enc, ids, mask), small["out"])
    assert torch.equal(enc(torch.from_numpy(ids), torch.from_numpy(mask).long()), small["out"])          # from the CPU, an integer mask
    for b in range(ids.shape[0]):
        assert torch.equal(_run(enc, ids[b:b + 1], mask[b:b + 1])[0], small["out"][b]), b
    none = _run(enc, ids, None)
    assert torch.equal(none, _run(enc, ids, np.ones_like(mask))) and not torch.equal(none, small["out"])


def test_causality_and_masked_positions(small):
    enc, ids, mask = small["enc"], small["ids"], small["mask"]
    t = 7
    later = ids.copy()
    later[:, t + 1:] = (later[:, t + 1:] + 1) % U.VOCAB
    out = _run(enc, later, mask)
    assert torch.equal(out[:, :t + 1], small["out"][:, :t + 1]) and not torch.equal(out[:, t + 1:], small["out"][:, t + 1:])
    under = ids.copy()
    under[~mask] = (under[~mask] + 1) % U.VOCAB
    out = _run(enc, under, mask)
    for b in range(ids.shape[0]):
        first = int(np.argmin(mask[b])) if not mask[b].all() else ids.shape[1]
        assert torch.equal(out[b, :first], small["out"][b, :first]), b
        assert first == ids.shape[1] or not torch.equal(out[b, first:], small["out"][b, first:]), b


def test_a_nan_embedding_under_masked_positions_is_never_read(small):
    """Parity-unpinned (torch multiplies the value under a masked key by a zero weight): held to the specification's rule only."""
    C, H, I, layers, B, T = small["shape"]
    params = U.make_params(C, I, layers)
    nan_id = 5
    params["text_model.embeddings.token_embedding.weight"][nan_id] = np.nan
    enc = U.build_encoder(C, H, I, layers, params=params).cuda()
    ids, mask = small["ids"].copy(), small["mask"]
    ids[ids == nan_id] = 6                                  # the NaN row is read nowhere ...
    clean = _run(enc, ids, mask)
    poisoned = ids.copy()
    poisoned[~mask] = nan_id                                # ... or only at masked positions
    out = _run(enc, poisoned, mask)
    for b in range(B):
        first = int(np.argmin(mask[b]))
        assert torch.isfinite(out[b, :first]).all() and torch.equal(out[b, :first], clean[b, :first]), b
        assert torch.isnan(out[b, first:]).all(), b         # the masked rows themselves are computed, from their own NaN


def test_an_id_outside_the_vocabulary(small):
    enc, ids, mask = small["enc"], small["ids"], small["mask"]
    for bad_id in (U.VOCAB, -1, 2 ** 40):
        bad = ids.copy()
        bad[2, 9] = bad_id
        out = _run(enc, bad, mask)                          # on the device: no error, no host wait; the row and what attends to it are NaN
        assert torch.isnan(out[2, 9:13]).all() and torch.equal(out[2, :9], small["out"][2, :9])
        assert torch.equal(out[[0, 1, 3]], small["out"][[0, 1, 3]])
        with pytest.raises(ValueError, match="outside"):
            enc(torch.from_numpy(bad), torch.from_numpy(mask))          # on the CPU it is checked there


def test_a_text_whose_first_token_is_masked_follows_the_zeros_rule(small):
    """Parity-unpinned: row 0 of text 1 has no admitted key; the attention gives zeros (``text_encoder_host.attention_host``)."""
    enc, ids = small["enc"], small["ids"]
    mask = small["mask"].copy()
    mask[1, 0] = False
    f64, f32 = enc.forward_host(ids, mask), enc.forward_host(ids, mask, dtype=np.float32)
    out = _run(enc, ids, mask)
    _held("mask[1,0] false", out.cpu().numpy(), f32, f64)
    assert not torch.equal(out[1, 0], small["out"][1, 0]) and torch.equal(out[0], small["out"][0])


def test_shapes_beyond_the_limits_raise(small):
    from proxytransformation_amd import ClipTextEncoder
    enc = small["enc"]
    with pytest.raises(ValueError, match="tokens"):
        enc(torch.zeros((1, U.POSITIONS + 1), dtype=torch.int64).cuda())
    with pytest.raises(ValueError, match="texts"):
        enc(torch.zeros((65, 4), dtype=torch.int64).cuda())
    with pytest.raises(ValueError, match="integer"):
        enc(torch.zeros((2, 4)).cuda())
    with pytest.raises(NotImplementedError, match="gelu"):
        ClipTextEncoder(hidden_act="gelu")
    with pytest.raises(ValueError, match="hidden_size"):
        ClipTextEncoder(hidden_size=1344, num_attention_heads=21)
    with pytest.raises(ValueError, match="intermediate_size"):
        ClipTextEncoder(intermediate_size=5184)


def test_prepared_operands_follow_the_parameters(small):
    C, H, I, layers, B, T = small["shape"]
    enc = U.build_encoder(C, H, I, layers).cuda()
    ids, mask = small["ids"], small["mask"]
    assert torch.equal(_run(enc, ids, mask), small["out"])
    other = U.make_params(C, I, layers, seed=1)
    enc.load_state_dict({k[len("text_model."):]: torch.from_numpy(v) for k, v in other.items()})
    out = _run(enc, ids, mask)
    assert not torch.equal(out, small["out"])
    _held("after load_state_dict", out.cpu().numpy(), enc.forward_host(ids, mask, dtype=np.float32), enc.forward_host(ids, mask))


# ------------------------------------------------------------------------------------------------------------------ the detector
ENC = dict(vocab_size=U.VOCAB, hidden_size=128, intermediate_size=128, num_hidden_layers=1, num_attention_heads=2)


@pytest.fixture(scope="module")
def world():
    x = inputs("cuda")
    det = make_detector(differentiable=True, text_encoder=dict(ENC)).cuda()
    ids = torch.from_numpy(U.make_ids(2, 12)).cuda()
    return dict(x=x, det=det, ids=ids, att=x["mask"].long())


def test_predict_takes_input_ids_in_place_of_the_encoded_text(world):
    x, det, ids, att = world["x"], world["det"].eval(), world["ids"], world["att"]
    got = det.predict(x["points"], img_features=x["img"], scenes=x["scenes"], img_pad_shape=PAD, input_ids=ids, attention_mask=att)
    text, mask = det.encode_text(ids, att)
    assert text.shape == (2, 12, 128) and mask.dtype == torch.bool and torch.equal(mask, x["mask"])
    assert torch.equal(text, det.text_encoder(ids, att))
    want = det.predict(x["points"], encoded_text=text, text_token_mask=att.bool(), img_features=x["img"], scenes=x["scenes"], img_pad_shape=PAD)
    for g, w in zip(got, want):
        assert g.keys() == w.keys() and all(torch.equal(g[k], w[k]) for k in g)
        assert torch.isfinite(g["bboxes_3d"]).all()


def test_loss_takes_input_ids_and_the_encoder_receives_no_gradient(world):
    x, det, ids, att = world["x"], world["det"].train(), world["ids"], world["att"]
    got = det.loss(x["points"], img_features=x["img"], scenes=x["scenes"], gt_bboxes=x["gt"], positive_maps=x["pos"], img_pad_shape=PAD,
                   input_ids=ids, attention_mask=att)
    sum(got.values()).backward()
    assert all(p.grad is None and not p.requires_grad for p in det.text_encoder.parameters())
    assert det.text_feat_map.weight.grad is not None and det.text_feat_map.weight.grad.abs().sum() > 0
    want = det.loss(x["points"], det.text_encoder(ids, att), att.bool(), x["img"], x["scenes"], x["gt"], x["pos"], img_pad_shape=PAD)
    assert got.keys() == want.keys() and all(torch.equal(got[k], want[k]) and torch.isfinite(got[k]) for k in got)
    det.zero_grad(set_to_none=True)


def test_reference_checkpoint_round_trip_with_the_text_encoder(world):
    x, det, ids, att = world["x"], world["det"].eval(), world["ids"], world["att"]
    sd = {k: v.detach().clone() for k, v in det.reference_state_dict().items()}
    assert sum(k.startswith("text_encoder.") for k in sd) == 2 + 16 + 2
    other = make_detector(differentiable=True, text_encoder=dict(ENC))
    with torch.no_grad():
        for p in other.text_encoder.parameters():
            p.zero_()
    other = other.cuda().eval()
    rep = other.load_reference_state_dict(sd)
    assert not [k for k in rep["skipped"] if k.startswith("text_encoder.")] and not rep["missing"] and not rep["unexpected"]
    kw = dict(img_features=x["img"], scenes=x["scenes"], img_pad_shape=PAD, input_ids=ids, attention_mask=att)
    for g, w in zip(other.predict(x["points"], **kw), det.predict(x["points"], **kw)):
        assert all(torch.equal(g[k], w[k]) for k in g)
