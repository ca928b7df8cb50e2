"""The device sampler of the multi-view ingest (``MultiViewIngest(sampler="device")``, ``ptx_ingest_draw``) on the GPU: its ``sel`` is
bit-identical to the host restatement ``ingest.device_choices``; the points it leads to are bit-identical to the host path fed the
same ``sel``; played through the oracle's two-stage ``PointSample`` the draws give the same cloud; the call never waits for the
device; the draws are reproducible from a seed or a scene's own ``draw_seed``; an all-empty scene is reported, not faulted; and the
chained ``GroundingFeaturePrefix`` in device mode equals the host mode fed the device draws."""
import contextlib

import numpy as np
import pytest
import torch

from proxytransformation_amd import _abi
from proxytransformation_amd.ingest import MultiViewIngest, device_choices, scene_key
from proxytransformation_amd.pipeline import GroundingFeaturePrefix
from proxytransformation_amd.synth import CONFIGS, FPN_LEVELS, PreshapeConfig, make_depth_scene
from tests.util import assert_close, build_module

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda:0")


def _to_dev(sc):
    d = sc["depth_img"]
    dt = torch.from_numpy(d.view(np.int16)).to(_dev()).view(torch.uint16) if d.dtype == np.uint16 else torch.from_numpy(d).to(_dev())
    return dict(depth_img=dt, depth_shift=float(sc.get("depth_shift", 1.0)), depth_cam2img=sc["depth_cam2img"],
                extrinsic=sc["extrinsic"])


def _counts(d):
    return (d.reshape(d.shape[0], -1) != 0).sum(1).astype(np.int64)


def _scene(seed, V, H, W, as_u16, variant=None):
    sc = make_depth_scene(seed, V=V, H=H, W=W, as_u16=as_u16)
    d = sc["depth_img"]
    if variant in ("zero_view", "sparse_view"):
        d[2] = 0                                                            # one view without a valid pixel
    if variant == "sparse_view":
        d[5].reshape(-1)[100:] = 0                                          # one view with fewer than per_view valid pixels
    return sc


def _aug():
    a = 0.3
    rot = np.array([[np.cos(a), np.sin(a), 0.0], [-np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]], np.float32)
    return dict(rot_mat_T=rot, scale=1.05, trans=np.array([0.1, -0.2, 0.05], np.float32))


@contextlib.contextmanager
def _count_waits():
    """Every Python-level way to drain the device / a stream / an event, and every ptx_wait_counts call, counted."""
    calls = []
    lib = _abi.lib()
    saved = (torch.cuda.synchronize, torch.cuda.Stream.synchronize, torch.cuda.Event.synchronize, lib.ptx_wait_counts)

    def wrap(name, fn):
        def inner(*a, **k):
            calls.append(name)
            return fn(*a, **k)
        return inner
    torch.cuda.synchronize = wrap("torch.cuda.synchronize", saved[0])
    torch.cuda.Stream.synchronize = wrap("Stream.synchronize", saved[1])
    torch.cuda.Event.synchronize = wrap("Event.synchronize", saved[2])
    lib.ptx_wait_counts = wrap("ptx_wait_counts", saved[3])
    try:
        yield calls
    finally:
        torch.cuda.synchronize, torch.cuda.Stream.synchronize, torch.cuda.Event.synchronize, lib.ptx_wait_counts = saved


CASES = [  # (V, H, W, N, per_view, variant)
    (50, 480, 640, 100000, None, None),                                     # the shipped shape: 50 x 480 x 640 -> 100 000
    (8, 120, 160, 20000, None, "zero_view"),
    (8, 120, 160, 20000, None, "sparse_view"),
    (8, 120, 160, 20000, 1000, "sparse_view"),                              # E * per_view = 7000 < N: the aggregate replaces
]


@pytest.mark.parametrize("as_u16", [True, False], ids=["u16", "f32"])
@pytest.mark.parametrize("case", range(len(CASES)), ids=["shipped", "zero_view", "sparse_view", "agg_replace"])
def test_device_sel_is_the_host_restatement(case, as_u16):
    V, H, W, N, pv, variant = CASES[case]
    scenes_np = [_scene(8100 + case, V, H, W, as_u16, variant), _scene(8200 + case, V, H, W, as_u16)]
    scenes = [_to_dev(s) for s in scenes_np]
    ing = MultiViewIngest(N, per_view_points=pv, sampler="device")
    batch = ing(scenes, seed=1234)
    torch.cuda.synchronize()
    batch.check()
    per_view = ing.per_view_points
    for b, sc in enumerate(scenes_np):
        key = scene_key(1234, b)
        assert batch.keys[b] == key and batch.sel[b] is None and batch.view_counts[b] is None
        want = device_choices(_counts(sc["depth_img"]), per_view, N, key)
        got = batch.sel_device[b].cpu().numpy()
        assert np.array_equal(got, want), (b, int((got != want).sum()))
    assert (batch.draw_status.cpu().numpy() == 0).all()


@pytest.mark.parametrize("with_aug", [False, True], ids=["plain", "aug"])
@pytest.mark.parametrize("as_u16", [True, False], ids=["u16", "f32"])
def test_device_points_equal_host_path_fed_the_device_sel(as_u16, with_aug):
    scenes = [_to_dev(_scene(8300 + b, 8, 240, 320, as_u16, "sparse_view" if b else None)) for b in range(2)]
    if with_aug:
        scenes = [dict(sc, aug=_aug()) for sc in scenes]
    dev_b = MultiViewIngest(20000, sampler="device")(scenes, seed=99)
    sel = [s.cpu().numpy() for s in dev_b.sel_device]
    host_b = MultiViewIngest(20000)([dict(sc, choices=sel[b]) for b, sc in enumerate(scenes)])
    for b in range(2):
        assert torch.equal(dev_b.points[b], host_b.points[b]), b
    assert torch.equal(dev_b.bbox, host_b.bbox)
    # a scene's own choices win in device mode as well (and its counts are then read as in the host path)
    mixed = MultiViewIngest(20000, sampler="device")([dict(scenes[0], choices=sel[0]), scenes[1]], seed=99)
    assert mixed.keys[0] is None and mixed.sel_device[0] is None and np.array_equal(mixed.sel[0], sel[0])
    assert torch.equal(mixed.points[0], dev_b.points[0])
    assert mixed.keys[1] == dev_b.keys[1] and torch.equal(mixed.points[1], dev_b.points[1])


class _StageRng:
    """Stand-in for np.random: ``choice`` hands out the device sampler's stages in the reference's order."""

    def __init__(self, stages, per_view, n_points):
        self.stages, self.i, self.per_view, self.n_points = list(stages), 0, per_view, n_points

    def choice(self, a, size, replace):
        st = self.stages[self.i]
        self.i += 1
        last = self.i == len(self.stages)
        assert size == (self.n_points if last else self.per_view) and len(st) == size
        assert replace == (len(a) < size)
        return np.asarray(a)[st]


@pytest.mark.parametrize("variant", [None, "sparse_view"])
def test_draws_through_the_oracles_two_point_samples(variant):
    """The composition is the reference's two-stage PointSample: the oracle fed the stages gives the same cloud (atol 1e-5)."""
    from oracle import oracle
    sc = _scene(8400, 8, 240, 320, True, variant)
    N = 20000
    batch = MultiViewIngest(N, sampler="device")([_to_dev(sc)], seed=5)
    d = sc["depth_img"]
    depth = d.astype(np.float32) / np.float32(sc["depth_shift"])
    sel, stages = device_choices(_counts(d), N // 10, N, batch.keys[0], return_stages=True)
    rng = _StageRng(stages, N // 10, N)
    ref = oracle.ingest(depth, sc["depth_cam2img"], sc["extrinsic"], N, rng=rng)
    assert rng.i == len(stages)
    assert np.array_equal(ref["sel"], batch.sel_device[0].cpu().numpy()) and np.array_equal(ref["sel"], sel)
    assert_close(batch.points[0].cpu().numpy(), ref["points"], atol=1e-5, what="device draws vs oracle")


def test_device_mode_call_never_waits():
    scenes = [_to_dev(_scene(8500 + b, 8, 240, 320, True)) for b in range(3)]
    ing = MultiViewIngest(20000, sampler="device")
    ing(scenes, seed=1)                                                     # warm-up: slots, workspaces
    torch.cuda.synchronize()
    with _count_waits() as calls:
        batch = ing(scenes, seed=2)
    assert calls == [], f"the device-mode ingest waited: {calls}"
    torch.cuda.synchronize()
    batch.check()
    # ... while the host mode waits once per scene for its per-view counts
    host = MultiViewIngest(20000)
    host(scenes, rng=np.random.RandomState(0))
    torch.cuda.synchronize()
    with _count_waits() as calls:
        host(scenes, rng=np.random.RandomState(0))
    assert calls.count("ptx_wait_counts") == 3
    torch.cuda.synchronize()


def test_determinism_and_draw_seed():
    a_np, b_np = _scene(8600, 8, 240, 320, True), _scene(8601, 8, 240, 320, False)
    a, b = _to_dev(a_np), _to_dev(b_np)
    ing = MultiViewIngest(20000, sampler="device")
    r1 = ing([a, b], seed=42)
    r1_pts = [p.clone() for p in r1.points]
    r2 = ing([a, b], seed=42)
    for k in range(2):
        assert torch.equal(r1_pts[k], r2.points[k]) and torch.equal(r1.sel_device[k], r2.sel_device[k])
    r3 = MultiViewIngest(20000, sampler="device")([a, b], seed=43)
    assert not torch.equal(r3.sel_device[0], r1.sel_device[0])
    # a seeded np.random reproduces a run: one 64-bit draw per call
    np.random.seed(7)
    r4 = [p.clone() for p in ing([a, b]).points]
    np.random.seed(7)
    r5 = ing([a, b])
    assert all(torch.equal(r4[k], r5.points[k]) for k in range(2))
    # draw_seed: the scene's cloud does not depend on its position in the batch
    x = ing([dict(a, draw_seed=2024), b], seed=1)
    x0 = x.points[0].clone()
    y = ing([b, dict(a, draw_seed=2024)], seed=1)
    assert torch.equal(x0, y.points[1]) and y.keys[1] == 2024
    # without it, position b gets its own key
    z = ing([a, a], seed=1)
    assert z.keys[0] != z.keys[1] and not torch.equal(z.sel_device[0], z.sel_device[1])
    want = device_choices(_counts(a_np["depth_img"]), 2000, 20000, 2024)
    assert np.array_equal(y.sel_device[1].cpu().numpy(), want)


def test_all_empty_scene_is_reported():
    good = _to_dev(_scene(8700, 4, 120, 160, True))
    empty = dict(good, depth_img=torch.zeros_like(good["depth_img"]))
    batch = MultiViewIngest(5000, sampler="device")([good, empty], seed=3)
    torch.cuda.synchronize()
    st = batch.draw_status.cpu().numpy()
    assert st[0] == 0 and st[1] == 1
    assert (batch.sel_device[1].cpu().numpy() == 0).all()
    assert (batch.points[1].cpu().numpy() == 0).all()
    with pytest.raises(ValueError):
        batch.check()
    # the good scene is untouched by its neighbour
    alone = MultiViewIngest(5000, sampler="device")([good], seed=3)
    assert torch.equal(alone.points[0], batch.points[0])
    alone.check()


def test_pipeline_device_mode_equals_host_mode_fed_the_device_draws():
    base = CONFIGS["cfg4_room"]
    cfg = PreshapeConfig("pipe_dev", B=2, N=20000, grid_size=base.grid_size, dynamic_drop_radio=base.dynamic_drop_radio,
                         L=base.L, V=8, text_blocks=3, img_blocks=3, extent=base.extent, seed_base=8800)
    m, _ = build_module(cfg)
    m = m.cuda()
    dev = _dev()
    scenes_np = [make_depth_scene(8800 + b, V=8, as_u16=True) for b in range(2)]
    scenes = []
    for sc in scenes_np:
        d = sc["depth_img"]
        scenes.append(dict(sc, depth_img=torch.from_numpy(d.view(np.int16)).to(dev).view(torch.uint16)))
    g = torch.Generator(device=dev)
    g.manual_seed(8800)
    feats = [torch.randn((2, 8, c, s, s), generator=g, device=dev, dtype=torch.float32) for c, s in FPN_LEVELS]
    text = {"text_feats": torch.randn((2, cfg.L, cfg.embed_dim), generator=g, device=dev),
            "text_token_mask": torch.ones((2, cfg.L), dtype=torch.bool, device=dev)}
    pipe_d = GroundingFeaturePrefix(m, n_points=cfg.N, sampler="device")
    pipe_h = GroundingFeaturePrefix(m, n_points=cfg.N)
    pipe_d(scenes, text, feats, seed=11)                                   # warm-up
    pipe_h(scenes, text, feats, rng=np.random.RandomState(0))
    torch.cuda.synchronize()
    with _count_waits() as calls_h:
        pipe_h(scenes, text, feats, rng=np.random.RandomState(0))
    torch.cuda.synchronize()
    with _count_waits() as calls_d:
        res_d = pipe_d(scenes, text, feats, seed=11)
    torch.cuda.synchronize()
    m.check()
    # no synchronise anywhere; of the count waits only the later stages' row counts remain (the ingest's one per scene is gone)
    assert [c for c in calls_d if c != "ptx_wait_counts"] == [], calls_d
    assert calls_d.count("ptx_wait_counts") == calls_h.count("ptx_wait_counts") - 2, (calls_d, calls_h)
    res_d.ingested.check()
    sel = [s.cpu().numpy() for s in res_d.ingested.sel_device]
    res_h = pipe_h([dict(sc, choices=sel[b]) for b, sc in enumerate(scenes)], text, feats)
    torch.cuda.synchronize()
    for b in range(2):
        assert torch.equal(res_d.ingested.points[b], res_h.ingested.points[b])
        assert torch.equal(res_d.points[b], res_h.points[b])
    assert torch.equal(res_d.coordinates, res_h.coordinates) and res_d.scene_rows == res_h.scene_rows
    for li in range(4):
        for b in range(2):
            assert torch.equal(res_d.level_coords[li][b], res_h.level_coords[li][b])
            assert torch.equal(res_d.points_imgfeats[b][li], res_h.points_imgfeats[b][li])
