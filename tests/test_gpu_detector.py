"""``GroundingDetector`` on the GPU: the seams (the detector against the existing modules called one by one with torch glue, bit for
bit, forward and backward, fused join and per-scene route), the oracle chain (the device against ``forward_host`` in float64 with the
device's decisions replayed, bounded by 4 x what ``forward_host`` in float32 differs from it), the train-mode and eval-mode behaviour,
and the checkpoint round trip.

Shape: two scenes of 4096 points in a room of 2 m, 3 views, 96 x 96 padded images (feature maps 24, 12, 6 and 3 pixels wide),
MinkResNet-18, ``pts_prune_threshold`` 200, 32 queries, 2 decoder layers, 12 text tokens of which some are masked, 1 and 3 boxes.
The fixture asserts what the shape is chosen for: every level of both scenes is non-empty, a prune step drops rows, and
``num_queries`` is smaller than the smallest scene's rows."""
import copy

import numpy as np
import pytest
import torch

from oracle import oracle

from tests.detector_util import B, N, PAD, V, inputs, make_detector

pytestmark = pytest.mark.gpu

def _manual(det, x, img, text, trace):
    """The existing modules one by one with torch glue -- what a user had to write: DET:385-482 with ``batch_point_sample`` per scene
    and level and the two ``torch.cat``, then DET:486-621 and the head."""
    from proxytransformation_amd.backbone import SparseLevel
    from proxytransformation_amd.decoder import linear
    from proxytransformation_amd.fusion import batch_point_sample
    from proxytransformation_amd.pipeline import projection_matrices
    d = det.differentiable and det.training
    tf = linear(text, det.text_feat_map.weight, det.text_feat_map.bias, differentiable=d)
    td = dict(text_feats=tf, text_token_mask=x["mask"])
    outs = det.preshape(x["points"], td, img[-1])
    coords, feats, ends = det.preshape.quantize(outs, det.voxel_size, return_scene_rows=True)
    levels = det.backbone_3d(coords, ends, feats)
    joined = []
    for l, lv in enumerate(levels):
        lo = [0] + list(lv.scene_rows[:-1])
        parts = []
        for b, sc in enumerate(x["scenes"]):
            meta = sc.get("img_meta") or {}
            proj = torch.from_numpy(projection_matrices(sc["depth2img"])).cuda()
            pts = lv.coords[lo[b]:lv.scene_rows[b], 1:4].float() * det.voxel_size
            parts.append(batch_point_sample(meta, img[l][b], pts, proj, det.coord_type,
                                            img_scale_factor=meta["scale_factor"][:2] if "scale_factor" in meta else 1.0,
                                            img_crop_offset=meta.get("img_crop_offset", 0.0), img_flip=bool(meta.get("flip", False)),
                                            img_pad_shape=PAD, img_shape=tuple(meta.get("img_shape", PAD))[:2], aligned=False))
        joined.append(SparseLevel(feats=torch.cat([lv.feats, torch.cat(parts)], 1), coords=lv.coords, scene_rows=list(lv.scene_rows),
                                  tensor_stride=lv.tensor_stride))
    keep = []
    nf, ns, nx = det.neck_3d(joined, B, keep_out=keep)
    sel = {}
    dec, head = det.query_select(nf, ns, nx, tf, x["mask"], keep_out=sel)
    hidden, boxes = det.decoder(query=dec["query"], key=dec["feats"], value=dec["feats"], key_padding_mask=dec["feats_attention_mask"],
                                self_attn_mask=None, cross_attn_mask=None, query_coords=dec["query_coords"], key_coords=dec["feats_coords"],
                                pred_bboxes=dec["pred_bboxes"], text_feats=dec["text_feats"], text_attention_mask=dec["text_attention_mask"],
                                bbox_head=det.query_select)
    scores = det.decoder.head_scores(hidden, dict(head, hidden_states=hidden), det.query_select, differentiable=d)
    trace.update(text_feats=tf, points=outs, coordinates=coords, features=feats, scene_rows=ends, levels=levels, joined=joined,
                 neck=(nf, ns, nx), keep=keep, select=sel, decoder_inputs=dec)
    return dict(hidden_states=hidden, all_layers_pred_bboxes=boxes, all_layers_cls_scores=scores)


def _train_step(det, x, route):
    """One loss + backward on a copy of ``det``; returns the losses, the trace and every gradient."""
    det = copy.deepcopy(det).train()
    det.fused_join = route == "fused"
    img = [f.detach().clone().requires_grad_() for f in x["img"]]
    text = x["text"].detach().clone().requires_grad_()
    trace = {}
    if route == "manual":
        head = _manual(det, x, img, text, trace)
        losses = det.bbox_head.loss(head["all_layers_cls_scores"], head["all_layers_pred_bboxes"], x["mask"], x["gt"], x["pos"])
    else:
        losses = det.loss(x["points"], text, x["mask"], img, x["scenes"], x["gt"], x["pos"], img_pad_shape=PAD, trace=trace)
    sum(losses.values()).backward()
    grads = {n: p.grad for n, p in det.named_parameters()}
    return dict(det=det, losses=losses, trace=trace, grads=grads, dtext=text.grad, dimg=[f.grad for f in img])


@pytest.fixture(scope="module")
def world():
    x = inputs("cuda")
    det = make_detector(differentiable=True).cuda()
    steps = {route: _train_step(det, x, route) for route in ("fused", "per_scene", "manual")}
    ev = copy.deepcopy(det).eval()
    pred, ptrace = {}, {}
    for route in ("fused", "per_scene"):
        ev.fused_join = route == "fused"
        ptrace[route] = {}
        pred[route] = ev.predict(x["points"], x["text"], x["mask"], x["img"], x["scenes"], img_pad_shape=PAD, trace=ptrace[route])
    mtrace = {}
    with torch.no_grad():
        mhead = _manual(ev, x, x["img"], x["text"], mtrace)
    torch.cuda.synchronize()
    return dict(x=x, det=det, steps=steps, ev=ev, pred=pred, ptrace=ptrace, mhead=mhead, mtrace=mtrace)


def _same(a, b, what):
    if isinstance(a, (list, tuple)):
        assert len(a) == len(b), what
        for i, (p, q) in enumerate(zip(a, b)):
            _same(p, q, f"{what}[{i}]")
    elif isinstance(a, dict):
        assert a.keys() == b.keys(), what
        for k in a:
            _same(a[k], b[k], f"{what}.{k}")
    elif isinstance(a, torch.Tensor):
        assert a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b), what
    elif hasattr(a, "feats") and hasattr(a, "coords"):
        _same(a.feats, b.feats, what + ".feats")
        _same(a.coords, b.coords, what + ".coords")
        assert list(a.scene_rows) == list(b.scene_rows) and a.tensor_stride == b.tensor_stride, what
    else:
        assert a == b, what


TRACED = ("text_feats", "points", "coordinates", "features", "scene_rows", "levels", "joined", "neck", "keep", "select", "decoder_inputs")


def test_the_shape_reaches_what_it_is_chosen_for(world):
    tr = world["steps"]["fused"]["trace"]
    for lv in tr["joined"]:
        rows = np.diff([0] + list(lv.scene_rows))
        print(f"stride {lv.tensor_stride}: rows per scene {rows.tolist()}, width {lv.feats.shape[1]}")
        assert (rows > 0).all(), "every level of both scenes is non-empty"
    assert any(int(k.numel()) > int(k.sum()) for k in tr["keep"]), "at least one prune step drops rows"
    smallest = min(int(f.shape[0]) for f in tr["neck"][0])
    print("rows per scene behind the neck:", [int(f.shape[0]) for f in tr["neck"][0]])
    assert tr["decoder_inputs"]["query"].shape[1] == 32 < smallest


def test_seams_training_forward_backward_bit_for_bit(world):
    """The detector's loss, every intermediate, every parameter's gradient and the gradients of ``encoded_text`` and all four levels
    of ``img_features`` equal the modules called one by one; the fused join and the per-scene route give equal bits."""
    ref = world["steps"]["manual"]
    for route in ("fused", "per_scene"):
        got = world["steps"][route]
        _same(got["losses"], ref["losses"], f"{route}: losses")
        for k in TRACED:
            _same(got["trace"][k], ref["trace"][k], f"{route}: {k}")
        assert got["grads"].keys() == ref["grads"].keys()
        none = sorted(n for n, g in got["grads"].items() if g is None)
        print(f"{route}: parameters without a gradient: {none}")
        # what the reference does not train either: the neck's score head feeds the prune alone, under no_grad (mink_neck.py:163-186),
        # and the decoder layers' own self_posembed is never read
        assert all(n.startswith("neck_3d.conv_cls.") or (n.startswith("decoder.layers.") and ".self_posembed." in n) for n in none), none
        for n, g in got["grads"].items():
            if g is None:
                assert ref["grads"][n] is None, f"{route}: {n} has a gradient in the reference chain only"
            else:
                assert torch.equal(g, ref["grads"][n]), f"{route}: grad of {n}"
        _same(got["dtext"], ref["dtext"], f"{route}: grad of encoded_text")
        _same(got["dimg"], ref["dimg"], f"{route}: grad of img_features")
    got = world["steps"]["fused"]
    assert set(got["losses"]) == {"loss_cls", "loss_bbox", "d0.loss_cls", "d0.loss_bbox"}
    assert all(torch.isfinite(v) for v in got["losses"].values())
    assert got["dtext"].abs().sum() > 0 and all(g is not None and g.abs().sum() > 0 for g in got["dimg"])
    assert all(g.abs().sum() > 0 for n, g in got["grads"].items() if n.endswith("weight") and "backbone_3d.layer" in n)


def test_seams_eval_predict_bit_for_bit(world):
    boxes, scores = world["ev"].bbox_head.predict(world["mhead"]["all_layers_cls_scores"], world["mhead"]["all_layers_pred_bboxes"])
    for route in ("fused", "per_scene"):
        pred = world["pred"][route]
        assert len(pred) == B
        for b in range(B):
            assert pred[b]["bboxes_3d"].shape == (32, 9) and pred[b]["scores_3d"].shape == (32,)
            assert torch.equal(pred[b]["bboxes_3d"], boxes[b]) and torch.equal(pred[b]["scores_3d"], scores[b])
            assert torch.equal(pred[b]["target_scores_3d"], pred[b]["scores_3d"]) and pred[b]["bboxes_3d"].grad_fn is None
        for k in TRACED:
            _same(world["ptrace"][route][k], world["mtrace"][k], f"eval {route}: {k}")


def test_one_train_step_updates_every_batchnorm_once(world):
    before = {n: int(m.num_batches_tracked) for n, m in world["det"].named_modules() if isinstance(m, torch.nn.modules.batchnorm._BatchNorm)}
    assert before and all(v == 0 for v in before.values())
    after = {n: m for n, m in world["steps"]["fused"]["det"].named_modules() if isinstance(m, torch.nn.modules.batchnorm._BatchNorm)}
    assert after.keys() == before.keys()
    base = dict(world["det"].named_modules())
    for n, m in after.items():
        if n.startswith("decoder.layers.") and ".self_posembed." in n:       # loaded and never read, as in the reference
            assert int(m.num_batches_tracked) == 0, n
            continue
        # the decoder applies its two shared position embeddings in every layer (the reference's loop): one step counts NL batches
        want = world["det"].decoder.num_layers if n.startswith(("decoder.self_posembed.", "decoder.cross_posembed.")) else 1
        assert m.training and int(m.num_batches_tracked) == want, (n, int(m.num_batches_tracked), want)
        assert not torch.equal(m.running_mean, base[n].running_mean), n


def test_eval_with_an_input_requiring_grad_raises_the_childrens_error(world):
    x, ev = world["x"], world["ev"]
    with pytest.raises(NotImplementedError):
        ev.predict(x["points"], x["text"].detach().clone().requires_grad_(), x["mask"], x["img"], x["scenes"], img_pad_shape=PAD)
    plain = copy.deepcopy(ev)
    plain.differentiable = False
    img = [f.detach().clone().requires_grad_() for f in x["img"]]
    with pytest.raises(NotImplementedError):
        plain.predict(x["points"], x["text"], x["mask"], img, x["scenes"], img_pad_shape=PAD)


def test_checkpoint_round_trip_reproduces_predict(world):
    x, ev = world["x"], world["ev"]
    other = make_detector(differentiable=True).cuda()
    with torch.no_grad():
        for p in other.parameters():
            p.mul_(0.5)
    other = other.eval()
    report = other.load_reference_state_dict({k: v.cpu() for k, v in ev.reference_state_dict().items()}, strict=True)
    assert not report["missing"] and not report["unexpected"]
    got = other.predict(x["points"], x["text"], x["mask"], x["img"], x["scenes"], img_pad_shape=PAD)
    _same(got, world["pred"]["fused"], "predict after the round trip")


def test_from_scenes_runs_the_ingest_in_front_of_predict(world):
    """Callers that hold depth maps: ``from_scenes`` gives the points and the bounding boxes that ``predict`` takes with the same scenes."""
    from proxytransformation_amd.synth import make_depth_scene
    x, ev = world["x"], world["ev"]
    raw = [make_depth_scene(900 + b, V=V, H=96, W=96, extent=(2.0, 2.0, 2.0)) for b in range(B)]
    scenes = [dict(sc, depth_img=torch.from_numpy(sc["depth_img"].view(np.int16)).cuda().view(torch.uint16)) for sc in raw]
    points, bbox = ev.from_scenes(scenes, n_points=N, rng=np.random.RandomState(0))
    assert len(points) == B and all(tuple(p.shape) == (N, 3) and p.is_cuda for p in points)
    got = ev.predict(points, x["text"], x["mask"], x["img"], scenes, img_pad_shape=PAD, bbox=bbox)
    assert len(got) == B
    for b in range(B):
        assert got[b]["bboxes_3d"].shape == (32, 9) and torch.isfinite(got[b]["bboxes_3d"]).all() and torch.isfinite(got[b]["scores_3d"]).all()


def _np(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def _tensors(r):
    """name -> array, the tensors the oracle chain is held on, from a device trace + head or from ``forward_host``'s dict."""
    out = {"text_feats": r["text_feats"], "features": r["features"]}
    for l, (lv, jl) in enumerate(zip(r["levels"], r["joined"])):
        out[f"backbone level {l}"], out[f"joined level {l}"] = lv.feats, jl.feats
    for b in range(B):
        out[f"neck feats {b}"], out[f"neck scores {b}"], out[f"neck points {b}"] = r["neck"][0][b], r["neck"][1][b], r["neck"][2][b]
    out["selection score"] = r["select"]["score"]
    for k in ("query", "feats", "query_coords", "feats_coords", "pred_bboxes"):
        out[f"decoder input {k}"] = r["decoder_inputs"][k]
    for k in ("hidden_states", "all_layers_pred_bboxes", "all_layers_cls_scores", "bboxes_3d", "scores_3d"):
        out[k] = r[k]
    for k, v in r["losses"].items():
        out[f"loss {k}"] = v
    return {k: np.asarray(_np(v), np.float64) for k, v in out.items()}


def test_oracle_chain_device_against_forward_host_float64(world):
    """The eval chain on the device against ``forward_host(float64)`` with the device's decisions replayed (the preshape's output
    clouds, the neck's keep masks, the query index, the matching).  The bound is not a constant: ``forward_host(float32)`` against
    ``forward_host(float64)`` on the same inputs and decisions gives, per tensor, the error of an fp32 chain relative to the tensor's
    scale (max |float64 value| over its finite entries); the device, another fp32 chain that differs in summation order, may be at
    most 4 x that (the margin the stage tests use for that difference).  Both columns are printed (profiles/detector.txt keeps them;
    measured on an MI355X: worst ratio 1.94 at the boxes handed to the decoder, every other tensor at or below 1.01)."""
    x, ev = world["x"], world["ev"]
    tr = world["ptrace"]["fused"]
    with torch.no_grad():
        head = ev.forward(x["points"], x["text"], x["mask"], x["img"], x["scenes"], img_pad_shape=PAD)
        losses = ev.bbox_head.loss(head["all_layers_cls_scores"], head["all_layers_pred_bboxes"], x["mask"], x["gt"], x["pos"])
        assign = ev.bbox_head.assign(head["all_layers_cls_scores"], head["all_layers_pred_bboxes"], x["mask"], x["gt"], x["pos"])
    pred = world["pred"]["fused"]
    dev = dict(tr, hidden_states=head["hidden_states"], all_layers_pred_bboxes=head["all_layers_pred_bboxes"],
               all_layers_cls_scores=head["all_layers_cls_scores"], bboxes_3d=torch.stack([p["bboxes_3d"] for p in pred]),
               scores_3d=torch.stack([p["scores_3d"] for p in pred]), losses=losses)
    decisions = dict(points=[_np(p) for p in tr["points"]], keep=[_np(k) for k in tr["keep"]], index=_np(tr["select"]["index"]),
                     assign=_np(assign))
    cpu = copy.deepcopy(ev).cpu()
    xc = {k: ([t.cpu() for t in v] if isinstance(v, list) and isinstance(v[0], torch.Tensor) else v.cpu() if isinstance(v, torch.Tensor) else v)
          for k, v in x.items()}
    host = {dt: cpu.forward_host(xc["points"], xc["text"], xc["mask"], xc["img"], xc["scenes"], img_pad_shape=PAD, dtype=dt,
                                 decisions=decisions, gt_bboxes=xc["gt"], positive_maps=xc["pos"], host=oracle) for dt in (np.float64, np.float32)}
    # the decisions that have ONE answer: the voxel rows
    assert np.array_equal(_np(tr["coordinates"]), host[np.float64]["coordinates"]) and list(tr["scene_rows"]) == list(host[np.float64]["scene_rows"])
    for lv, hl in zip(tr["levels"], host[np.float64]["levels"]):
        assert np.array_equal(_np(lv.coords), hl.coords) and list(lv.scene_rows) == list(hl.scene_rows)
    own = host[np.float64]
    print("host's own decisions against the device's: keep masks equal at", [int((_np(a) == b).sum()) for a, b in zip(tr["keep"], own["keep"])],
          "of", [int(b.size) for b in own["keep"]], "rows; query index equal at", int((_np(tr["select"]["index"]) == own["select"]["index"]).sum()),
          "of", own["select"]["index"].size)
    d, h64, h32 = _tensors(dev), _tensors(host[np.float64]), _tensors(host[np.float32])
    print(f"{'tensor':<38}{'scale':>11}{'float32 host':>14}{'device':>12}{'device / float32':>18}")
    bad = []
    for k, ref in h64.items():
        assert d[k].shape == ref.shape == h32[k].shape, (k, d[k].shape, ref.shape)
        fin = np.isfinite(ref)
        assert np.array_equal(fin, np.isfinite(d[k])) and np.array_equal(fin, np.isfinite(h32[k])), f"{k}: the -inf columns differ"
        scale = float(np.abs(ref[fin]).max()) or 1.0
        e32 = float(np.abs(h32[k][fin] - ref[fin]).max()) / scale
        ed = float(np.abs(d[k][fin] - ref[fin]).max()) / scale
        print(f"{k:<38}{scale:>11.3e}{e32:>14.3e}{ed:>12.3e}{(ed / e32 if e32 else float('inf') if ed else 0.0):>18.2f}")
        if ed > 4.0 * e32:
            bad.append((k, ed, e32))
    assert not bad, f"device error above 4 x the float32 chain's: {bad}"
