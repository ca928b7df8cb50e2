"""BASELINE configs[3] chained (GroundingFeaturePrefix, six cfg4_room scenes of 50 x 480 x 640 -> 100 000 points) with the two
PointSample draws precomputed on the host (`choices`, bench.py's method) against the device sampler (sampler="device"), A/B in one
process: warm-up, then `steps` chained calls between synchronises per block, five blocks, median; blocks of the two modes alternate.
Then the ingest stage alone per mode (time_stages=True, median of 11 calls), the host-drawing call (np.random.choice, 2 calls), and
the device mode's wait count.  usage: python scratch/ingest_device_draws.py [steps]"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.getcwd())
from proxytransformation_amd import _abi
from proxytransformation_amd.pipeline import GroundingFeaturePrefix
from proxytransformation_amd.synth import CONFIGS, FPN_LEVELS, make_depth_scene
from tests.util import build_module

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
cfg = CONFIGS["cfg4_room"]
dev = torch.device("cuda:0")
m, _ = build_module(cfg)
m = m.cuda()
B, V = 6, cfg.V
scenes = []
for b in range(B):
    sc = make_depth_scene(cfg.seed_base + 50 + b, V=V)
    scenes.append(dict(sc, depth_img=torch.from_numpy(sc["depth_img"].view(np.int16)).to(dev).view(torch.uint16)))
g = torch.Generator(device=dev)
g.manual_seed(cfg.seed_base)
feats = [torch.randn((B, V, c, s, s), generator=g, device=dev) for c, s in FPN_LEVELS]
text = {"text_feats": torch.randn((B, cfg.L, cfg.embed_dim), generator=g, device=dev),
        "text_token_mask": torch.ones((B, cfg.L), dtype=torch.bool, device=dev)}
pipe_h = GroundingFeaturePrefix(m, n_points=cfg.N)
pipe_d = GroundingFeaturePrefix(m, n_points=cfg.N, sampler="device")
with torch.no_grad():
    first = pipe_h(scenes, text, feats, rng=np.random.RandomState(0))
    pre = [dict(sc, choices=first.ingested.sel[b]) for b, sc in enumerate(scenes)]
    modes = {"host_precomputed": lambda i: pipe_h(pre, text, feats),
             "device": lambda i: pipe_d(scenes, text, feats, seed=i)}
    for name, f in modes.items():
        for i in range(5):
            f(i)
    torch.cuda.synchronize()
    m.check()
    blocks = {k: [] for k in modes}
    for r in range(5):
        for name, f in modes.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(steps):
                f(i)
            torch.cuda.synchronize()
            blocks[name].append(1e3 * (time.perf_counter() - t0) / steps)
    m.check()
    print(f"GroundingFeaturePrefix, {B} cfg4_room scenes ({V} x 480 x 640 -> {cfg.N}), {steps} chained calls per block, 5 blocks")
    for name, v in blocks.items():
        print(f"  {name:18s} median {sorted(v)[2]:8.3f} ms/call   blocks " + " ".join(f"{x:.3f}" for x in v))
    # the ingest stage alone (events between the stages of one call)
    for name, f in (("host_precomputed", lambda i: pipe_h(pre, text, feats, time_stages=True)),
                    ("device", lambda i: pipe_d(scenes, text, feats, seed=i, time_stages=True))):
        st = {}
        for i in range(11):
            for k, val in f(i).stage_ms.items():
                st.setdefault(k, []).append(val)
        print(f"  stages {name:18s} " + "  ".join(f"{k} {sorted(val)[5]:.3f}" for k, val in st.items()) + "  (ms, median of 11)")
    # the call drawing the pixels itself with np.random.choice (the reference's order)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(2):
        pipe_h(scenes, text, feats, rng=np.random.RandomState(i))
    torch.cuda.synchronize()
    print(f"  host_np_random     {1e3 * (time.perf_counter() - t0) / 2:8.1f} ms/call (2 calls)")
    # the device mode waits for no per-view count: ptx_wait_counts calls per chained call, per mode
    lib = _abi.lib()
    orig = lib.ptx_wait_counts
    for name, f in modes.items():
        n = [0]

        def counted(*a, _o=orig, _n=n):
            _n[0] += 1
            return _o(*a)
        torch.cuda.synchronize()
        lib.ptx_wait_counts = counted
        try:
            f(0)
        finally:
            lib.ptx_wait_counts = orig
        print(f"  ptx_wait_counts per call, {name}: {n[0]}")
    torch.cuda.synchronize()
    # the same outputs: device mode vs the host mode fed the device draws (last call's keys)
    rd = pipe_d(scenes, text, feats, seed=7)
    sel = [s.cpu().numpy() for s in rd.ingested.sel_device]
    rh = pipe_h([dict(sc, choices=sel[b]) for b, sc in enumerate(scenes)], text, feats)
    torch.cuda.synchronize()
    rd.ingested.check()
    same = torch.equal(rd.coordinates, rh.coordinates) and all(torch.equal(a, b) for a, b in zip(rd.points, rh.points))
    print(f"  device mode == host mode fed the device sel (points, voxel rows): {same}")
